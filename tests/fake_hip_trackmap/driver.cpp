// libdsdtm_amd_trackmap.so's host side (dsdtm_amd/csrc/trackmap_api.cpp) against the fake HIP runtime of tests/fake_hip (unmodified):
// the resident track map and its updates (staging ring, growth of the six arrays, retired arrays), the checks, the packing of a
// dsdtm_trackmap_local call, every failure path — under ASan/UBSan/LSan. The launches are the fakes of
// tests/fake_hip_trackmap/fake_trackmap.cpp and, for the selection, tests/fake_hip_localmap/fake_localmap.cpp. Test infrastructure
// (tests/test_track_map_fake_hip_cpu.py); nothing here is part of the product.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_trackmap.h"
#include "../../dsdtm_amd/host/dsdtm_trackmap_host.hpp"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_localmap.h"
#include "fake_trackmap.h"
#include "trackmap.h"

static const dsdtm_camera CAM{512.f, 512.f, 320.f, 240.f, 512.f, 640, 480};
static const double I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

// the host's mirror of a map
struct Mirror {
    std::vector<double> p, T, bearing;
    std::vector<uint8_t> bad, observes;
    std::vector<int32_t> found, ns, slots, level;
    std::vector<float> px;
    std::vector<int64_t> off;
    unsigned rng = 4321;
    unsigned next() { rng = rng * 1664525u + 1013904223u; return rng >> 8; }
    int P() const { return (int)bad.size(); }
    int K() const { return (int)ns.size(); }
    DSDTM::TrackMapArrays arrays() const {
        DSDTM::TrackMapArrays m;
        m.sel.n_points = P(); m.sel.p_world = p.data(); m.sel.bad = bad.data(); m.sel.n_keyframes = K(); m.sel.T_kf_w = T.data(); m.sel.n_slots = ns.data();
        m.sel.slot_offset = off.data(); m.sel.point_of_slot = slots.data();
        m.found = found.data(); m.observes = observes.data(); m.px_xy = px.data(); m.level = level.data(); m.bearing = bearing.data();
        return m;
    }
};

// the slot columns of one keyframe (or of a run of slots), drawn by the mirror's generator
struct Slots {
    std::vector<int32_t> s, level;
    std::vector<uint8_t> o;
    std::vector<float> px;
    std::vector<double> bearing;
};

struct World {
    dsdtm_trackmap_ctx* ctx = nullptr;
    dsdtm_trackmap* map = nullptr;
    Mirror m;
    bool points(int n, bool flags = true) {
        std::vector<double> x(3 * (size_t)n);
        std::vector<uint8_t> b((size_t)n);
        std::vector<int32_t> f((size_t)n);
        for (int i = 0; i < n; ++i) {
            x[3 * (size_t)i] = (double)(m.next() % 200) / 100.0 - 1.0; x[3 * (size_t)i + 1] = (double)(m.next() % 100) / 100.0 - 0.5;
            x[3 * (size_t)i + 2] = (double)(m.next() % 500) / 100.0 - 1.0;
            b[(size_t)i] = flags && m.next() % 10 == 0; f[(size_t)i] = flags ? (int32_t)(m.next() % 90) : 0;
        }
        std::vector<double> xs = x;
        std::vector<uint8_t> bs = b;
        std::vector<int32_t> fs = f;
        CHECK(dsdtm_trackmap_points_write(ctx, map, m.P(), n, xs.data(), flags ? bs.data() : nullptr, flags ? fs.data() : nullptr) == DSDTM_OK);
        std::fill(xs.begin(), xs.end(), -99.0); std::fill(bs.begin(), bs.end(), 77); std::fill(fs.begin(), fs.end(), -7);      // the caller's buffers are free at once
        m.p.insert(m.p.end(), x.begin(), x.end()); m.bad.insert(m.bad.end(), b.begin(), b.end()); m.found.insert(m.found.end(), f.begin(), f.end());
        return true;
    }
    Slots draw(int n) {
        Slots c;
        for (int i = 0; i < n; ++i) {
            const int32_t s = m.P() == 0 || m.next() % 5 == 0 ? -1 : (int32_t)(m.next() % (unsigned)m.P());
            c.s.push_back(s); c.o.push_back(s >= 0 && m.next() % 4 != 0); c.level.push_back((int32_t)(m.next() % 4));
            c.px.push_back((float)(m.next() % 640)); c.px.push_back((float)(m.next() % 480) + 0.5f);
            for (int r = 0; r < 3; ++r) c.bearing.push_back((double)(m.next() % 1000) / 1000.0);
        }
        return c;
    }
    bool keyframe(int n_slots) {
        const Slots c = draw(n_slots);
        Slots cc = c;
        double T[12], Tc[12];
        memcpy(T, I12, sizeof T);
        T[3] = (double)(m.next() % 16) * 0.25; T[11] = (double)(m.next() % 4) * 0.5;
        memcpy(Tc, T, sizeof T);
        int k = -1;
        CHECK(dsdtm_trackmap_keyframe_add(ctx, map, Tc, n_slots, cc.s.data(), cc.o.data(), cc.px.data(), cc.level.data(), cc.bearing.data(), &k) == DSDTM_OK && k == m.K());
        std::fill(cc.s.begin(), cc.s.end(), 555); std::fill(cc.o.begin(), cc.o.end(), 9); std::fill(cc.px.begin(), cc.px.end(), -1.f); Tc[3] = -1e9;
        m.off.push_back((int64_t)m.slots.size()); m.ns.push_back(n_slots); m.T.insert(m.T.end(), T, T + 12);
        m.slots.insert(m.slots.end(), c.s.begin(), c.s.end()); m.observes.insert(m.observes.end(), c.o.begin(), c.o.end());
        m.px.insert(m.px.end(), c.px.begin(), c.px.end()); m.level.insert(m.level.end(), c.level.begin(), c.level.end());
        m.bearing.insert(m.bearing.end(), c.bearing.begin(), c.bearing.end());
        return true;
    }
    // the device map equals the mirror (map_read), and a local call on it equals the host functions on the mirror
    bool agrees(int n_local = 6, int cap = 64, int ocap = 96) {
        dsdtm_trackmap_image im{};
        CHECK(dsdtm_trackmap_map_read(ctx, map, &im) == DSDTM_OK && im.complete == (m.P() == 0 && m.K() == 0));
        CHECK(im.n_points == m.P() && im.n_keyframes == m.K() && im.n_slots_total == (int64_t)m.slots.size());
        Mirror r;
        r.p.resize(m.p.size() + 1); r.T.resize(m.T.size() + 1); r.bearing.resize(m.bearing.size() + 1); r.bad.resize(m.bad.size() + 1);
        r.observes.resize(m.observes.size() + 1); r.found.resize(m.found.size() + 1); r.ns.resize(m.ns.size() + 1); r.slots.resize(m.slots.size() + 1);
        r.level.resize(m.level.size() + 1); r.px.resize(m.px.size() + 1); r.off.resize(m.off.size() + 1);
        im.point_capacity = m.P(); im.keyframe_capacity = m.K(); im.slot_capacity = (int64_t)m.slots.size();
        im.p_world = r.p.data(); im.bad = r.bad.data(); im.found = r.found.data(); im.T_kf_w = r.T.data(); im.n_slots = r.ns.data(); im.slot_offset = r.off.data();
        im.point_of_slot = r.slots.data(); im.observes = r.observes.data(); im.px_xy = r.px.data(); im.level = r.level.data(); im.bearing = r.bearing.data();
        CHECK(dsdtm_trackmap_map_read(ctx, map, &im) == DSDTM_OK && im.complete == 1);
        r.p.pop_back(); r.T.pop_back(); r.bearing.pop_back(); r.bad.pop_back(); r.observes.pop_back(); r.found.pop_back(); r.ns.pop_back(); r.slots.pop_back();
        r.level.pop_back(); r.px.pop_back(); r.off.pop_back();
        CHECK(r.p == m.p && r.T == m.T && r.bad == m.bad && r.found == m.found && r.ns == m.ns && r.off == m.off && r.slots == m.slots);
        CHECK(r.observes == m.observes && r.px == m.px && r.level == m.level && r.bearing == m.bearing);
        Out a(n_local, cap, ocap), b(n_local, cap, ocap);
        dsdtm_localmap_params prm{n_local, 0};
        dsdtm_trackmap_desc d = a.desc(map, I12);
        dsdtm_trackmap_result res{};
        CHECK(dsdtm_trackmap_local(ctx, &CAM, &prm, 1, &d, &res) == DSDTM_OK);
        dsdtm_localmap_result sel{};
        int32_t n_obs = 0;
        const DSDTM::TrackMapArrays w = m.arrays();
        DSDTM::select_local_map_host(CAM, prm, w.sel, I12, b.kf.data(), b.kd.data(), cap, b.pt.data(), b.pk.data(), &sel);
        DSDTM::flatten_local_map_host(w, std::min(sel.n_points, cap), b.pt.data(), ocap, b.pw.data(), b.mf.data(), b.mb.data(), b.oo.data(), b.ok.data(),
                                      b.op.data(), b.ol.data(), b.ob.data(), &n_obs);
        CHECK(res.n_close == sel.n_close && res.n_kf == sel.n_kf && res.n_points == sel.n_points && res.overflow_points == sel.overflow);
        CHECK(res.n_obs == n_obs && res.overflow_obs == (n_obs > ocap));
        CHECK(a.same(b));
        return true;
    }
    // the twelve output arrays of one desc, filled with 0xA5 (what a call does not write stays)
    struct Out {
        std::vector<int32_t> kf, pt, pk, mf, oo, ok, ol;
        std::vector<double> kd, pw, ob;
        std::vector<uint8_t> mb;
        std::vector<float> op;
        Out(int n_local, int cap, int ocap) : kf((size_t)n_local), pt((size_t)cap + 1), pk((size_t)cap + 1), mf((size_t)cap + 1), oo((size_t)cap + 2), ok((size_t)ocap + 1),
              ol((size_t)ocap + 1), kd((size_t)n_local), pw(3 * (size_t)cap + 3), ob(3 * (size_t)ocap + 3), mb((size_t)cap + 1), op(2 * (size_t)ocap + 2) { fill(); }
        void fill() {
            fill_a5(kf.data(), kf.size() * 4); fill_a5(pt.data(), pt.size() * 4); fill_a5(pk.data(), pk.size() * 4); fill_a5(mf.data(), mf.size() * 4);
            fill_a5(oo.data(), oo.size() * 4); fill_a5(ok.data(), ok.size() * 4); fill_a5(ol.data(), ol.size() * 4); fill_a5(kd.data(), kd.size() * 8);
            fill_a5(pw.data(), pw.size() * 8); fill_a5(ob.data(), ob.size() * 8); fill_a5(mb.data(), mb.size()); fill_a5(op.data(), op.size() * 4);
        }
        dsdtm_trackmap_desc desc(const dsdtm_trackmap* map, const double* T) {
            dsdtm_trackmap_desc d{};
            d.map = map; d.T_cur_w = T; d.point_capacity = (int32_t)pt.size() - 1; d.obs_capacity = (int32_t)ok.size() - 1;
            d.kf = kf.data(); d.kf_dist = kd.data(); d.point = pt.data(); d.point_kf = pk.data(); d.mp_world = pw.data(); d.mp_found = mf.data(); d.mp_bad = mb.data();
            d.obs_offset = oo.data(); d.obs_kf = ok.data(); d.obs_px = op.data(); d.obs_level = ol.data(); d.obs_bearing = ob.data();
            return d;
        }
        bool same(const Out& o) const {      // bytes: the written parts are equal and the rest is still the fill
            auto eq = [](const void* x, const void* y, size_t n) { return n == 0 || memcmp(x, y, n) == 0; };
            return eq(kf.data(), o.kf.data(), kf.size() * 4) && eq(pt.data(), o.pt.data(), pt.size() * 4) && eq(pk.data(), o.pk.data(), pk.size() * 4) &&
                   eq(mf.data(), o.mf.data(), mf.size() * 4) && eq(oo.data(), o.oo.data(), oo.size() * 4) && eq(ok.data(), o.ok.data(), ok.size() * 4) &&
                   eq(ol.data(), o.ol.data(), ol.size() * 4) && eq(kd.data(), o.kd.data(), kd.size() * 8) && eq(pw.data(), o.pw.data(), pw.size() * 8) &&
                   eq(ob.data(), o.ob.data(), ob.size() * 8) && eq(mb.data(), o.mb.data(), mb.size()) && eq(op.data(), o.op.data(), op.size() * 4);
        }
        bool untouched() const { Out f((int)kf.size(), (int)pt.size() - 1, (int)ok.size() - 1); return same(f); }
    };
    bool open() {
        CHECK(dsdtm_trackmap_create(0, &ctx) == DSDTM_OK && dsdtm_trackmap_map_create(ctx, &map) == DSDTM_OK);
        return true;
    }
    void close() { dsdtm_trackmap_map_destroy(ctx, map); dsdtm_trackmap_destroy(ctx); ctx = nullptr; map = nullptr; }
};

// the life of a map: many updates with no wait between them (the pinned ring), growth of all six arrays, rewrites
static bool updates_and_growth() {
    World w;
    CHECK(w.open() && w.agrees());
    CHECK(w.points(1) && w.points(63, false) && w.points(300) && w.agrees());
    CHECK(w.keyframe(0) && w.keyframe(1) && w.keyframe(300) && w.agrees());
    const long waits = fake_hip_calls("hipStreamSynchronize"), applied = fake_trackmap_update_launches();
    for (int i = 0; i < 40; ++i) CHECK(w.points(100) && w.keyframe(420));     // across the initial capacities; the library waits for nothing
    CHECK(fake_trackmap_update_launches() == applied + 80);                     // ONE launch per update
    CHECK(fake_hip_calls("hipStreamSynchronize") - waits == 80);                // (the fake launches' own drains, one each: none by the library)
    CHECK(w.m.P() > dsdtm::LM_INITIAL_POINTS && (int64_t)w.m.slots.size() > dsdtm::LM_INITIAL_SLOTS);
    CHECK(w.agrees());
    while (w.m.K() <= dsdtm::LM_INITIAL_KEYFRAMES) CHECK(w.keyframe(3));
    CHECK(w.agrees());
    for (int i = 0; i < 12; ++i) CHECK(w.points(4000));                        // more staged bytes than the pinned block holds: the ring wraps behind a wait
    CHECK(w.agrees());
    // rewrites: a pose, slots with their flags, pose and slots together, points with and without flags, found counts
    double T[12];
    memcpy(T, I12, sizeof T);
    T[3] = 0.125;
    CHECK(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 2, T, 0, 0, nullptr, nullptr) == DSDTM_OK);
    memcpy(&w.m.T[24], T, sizeof T);
    Slots c = w.draw(50);
    CHECK(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 2, nullptr, 250, 50, c.s.data(), c.o.data()) == DSDTM_OK);
    std::copy(c.s.begin(), c.s.end(), w.m.slots.begin() + w.m.off[2] + 250); std::copy(c.o.begin(), c.o.end(), w.m.observes.begin() + w.m.off[2] + 250);
    c = w.draw(7);
    T[11] = 3.0;
    CHECK(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 5, T, 10, 7, c.s.data(), c.o.data()) == DSDTM_OK);
    memcpy(&w.m.T[60], T, sizeof T);
    std::copy(c.s.begin(), c.s.end(), w.m.slots.begin() + w.m.off[5] + 10); std::copy(c.o.begin(), c.o.end(), w.m.observes.begin() + w.m.off[5] + 10);
    const double x[6] = {0.5, 0.25, 2.0, -0.5, 0.0, 3.0};
    const uint8_t b[2] = {1, 0};
    const int32_t f[2] = {41, -2};
    CHECK(dsdtm_trackmap_points_write(w.ctx, w.map, 17, 2, x, b, f) == DSDTM_OK);
    std::copy(x, x + 6, w.m.p.begin() + 51); w.m.bad[17] = 1; w.m.bad[18] = 0; w.m.found[17] = 41; w.m.found[18] = -2;
    CHECK(dsdtm_trackmap_points_write(w.ctx, w.map, 17, 1, x + 3, nullptr, nullptr) == DSDTM_OK);      // NULL flags on a rewrite: unchanged
    std::copy(x + 3, x + 6, w.m.p.begin() + 51);
    CHECK(dsdtm_trackmap_points_write(w.ctx, w.map, 19, 1, x, b, nullptr) == DSDTM_OK);                // one of the two
    std::copy(x, x + 3, w.m.p.begin() + 57); w.m.bad[19] = 1;
    const int32_t idx[3] = {0, w.m.P() - 1, 17}, val[3] = {7, 2147483647, 0};
    CHECK(dsdtm_trackmap_found_write(w.ctx, w.map, 3, idx, val) == DSDTM_OK);
    for (int i = 0; i < 3; ++i) w.m.found[(size_t)idx[i]] = val[i];
    CHECK(w.agrees() && w.agrees(1) && w.agrees(64, 4096, 200) && w.agrees(6, 3, 2) && w.agrees(6, 0, 0));
    w.close();
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

static bool named_err(dsdtm_trackmap_ctx* ctx, int rc, const char* what) {
    if (rc != DSDTM_ERR_INVALID || !strstr(dsdtm_trackmap_last_error(ctx), what)) {
        std::fprintf(stderr, "expected INVALID naming '%s': rc %d, error '%s'\n", what, rc, dsdtm_trackmap_last_error(ctx));
        return false;
    }
    return true;
}

static bool found_write_refusals() {
    World w, other;
    CHECK(w.open() && other.open() && w.points(10) && w.agrees());
    const long copies = fake_hip_calls("hipMemcpyAsync"), launches = fake_trackmap_update_launches();
    int32_t idx[3] = {1, 4, 9}, val[3] = {5, 6, 7};
    auto named = [&](int rc, const char* what) { return named_err(w.ctx, rc, what); };
    CHECK(named(dsdtm_trackmap_found_write(w.ctx, nullptr, 3, idx, val), "map is NULL"));
    CHECK(named(dsdtm_trackmap_found_write(w.ctx, other.map, 3, idx, val), "not a map of this context"));
    CHECK(named(dsdtm_trackmap_found_write(w.ctx, w.map, -1, idx, val), "n is negative"));
    CHECK(named(dsdtm_trackmap_found_write(w.ctx, w.map, 3, nullptr, val), "index is NULL"));
    CHECK(named(dsdtm_trackmap_found_write(w.ctx, w.map, 3, idx, nullptr), "found is NULL"));
    idx[2] = 10; CHECK(named(dsdtm_trackmap_found_write(w.ctx, w.map, 3, idx, val), "index[2] = 10"));
    idx[2] = -1; CHECK(named(dsdtm_trackmap_found_write(w.ctx, w.map, 3, idx, val), "index[2] = -1"));
    idx[2] = 1; CHECK(named(dsdtm_trackmap_found_write(w.ctx, w.map, 3, idx, val), "index 1 occurs twice"));
    CHECK(dsdtm_trackmap_found_write(w.ctx, w.map, 0, nullptr, nullptr) == DSDTM_OK);
    CHECK(fake_hip_calls("hipMemcpyAsync") == copies && fake_trackmap_update_launches() == launches && w.agrees());
    idx[2] = 9;
    CHECK(dsdtm_trackmap_found_write(w.ctx, w.map, 3, idx, val) == DSDTM_OK);
    for (int i = 0; i < 3; ++i) w.m.found[(size_t)idx[i]] = val[i];
    CHECK(w.agrees());
    other.close(); w.close();
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// every refused call names its field and leaves the map and the outputs as they were; nothing is enqueued
static bool validation() {
    World w, other;
    CHECK(w.open() && other.open());
    CHECK(w.points(10) && w.keyframe(4) && w.keyframe(6) && w.agrees());
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const long copies = fake_hip_calls("hipMemcpyAsync");
    const long launches = fake_trackmap_update_launches() + fake_trackmap_flatten_launches() + fake_localmap_select_launches();
    auto named = [&](int rc, const char* what) { return named_err(w.ctx, rc, what); };
    double x[6] = {0, 0, 1, 0, 0, 2}, T[12];
    memcpy(T, I12, sizeof T);
    int32_t s[4] = {0, -1, 9, 3}, lv[4] = {0, 1, 2, 3};
    uint8_t o[4] = {1, 0, 1, 0};
    float px[8] = {0};
    double be[12] = {0};
    int k = -5;
    CHECK(named(dsdtm_trackmap_points_write(w.ctx, nullptr, 0, 1, x, nullptr, nullptr), "map"));
    CHECK(named(dsdtm_trackmap_points_write(w.ctx, other.map, 0, 1, x, nullptr, nullptr), "not a map of this context"));
    CHECK(named(dsdtm_trackmap_points_write(w.ctx, w.map, 11, 1, x, nullptr, nullptr), "gap"));
    CHECK(named(dsdtm_trackmap_points_write(w.ctx, w.map, -1, 1, x, nullptr, nullptr), "first"));
    CHECK(named(dsdtm_trackmap_points_write(w.ctx, w.map, 0, -1, x, nullptr, nullptr), "n is"));
    CHECK(named(dsdtm_trackmap_points_write(w.ctx, w.map, 10, 2, nullptr, nullptr, nullptr), "p_world is NULL"));
    CHECK(named(dsdtm_trackmap_points_write(w.ctx, w.map, 10, DSDTM_LOCALMAP_MAX_POINTS, x, nullptr, nullptr), "exceeds"));
    x[4] = inf; CHECK(named(dsdtm_trackmap_points_write(w.ctx, w.map, 10, 2, x, nullptr, nullptr), "p_world is not finite")); x[4] = 0;
    CHECK(dsdtm_trackmap_points_write(w.ctx, w.map, 3, 0, nullptr, nullptr, nullptr) == DSDTM_OK);            // n == 0: nothing
    auto add = [&](const double* Tk, int n, const int32_t* sl, const uint8_t* ob, const float* p, const int32_t* l, const double* b) {
        return dsdtm_trackmap_keyframe_add(w.ctx, w.map, Tk, n, sl, ob, p, l, b, &k);
    };
    CHECK(named(add(nullptr, 4, s, o, px, lv, be), "T_kf_w is NULL"));
    CHECK(named(add(T, 4, nullptr, o, px, lv, be), "point_of_slot is NULL"));
    CHECK(named(add(T, 4, s, nullptr, px, lv, be), "observes is NULL"));
    CHECK(named(add(T, 4, s, o, nullptr, lv, be), "px_xy is NULL"));
    CHECK(named(add(T, 4, s, o, px, nullptr, be), "level is NULL"));
    CHECK(named(add(T, 4, s, o, px, lv, nullptr), "bearing is NULL"));
    CHECK(named(add(T, -1, s, o, px, lv, be), "n_slots"));
    CHECK(named(add(T, DSDTM_LOCALMAP_MAX_SLOTS + 1, s, o, px, lv, be), "n_slots"));
    s[2] = 10; CHECK(named(add(T, 4, s, o, px, lv, be), "point_of_slot[2] = 10"));
    s[2] = -2; CHECK(named(add(T, 4, s, o, px, lv, be), "point_of_slot[2] = -2")); s[2] = 9;
    o[1] = 1; CHECK(named(add(T, 4, s, o, px, lv, be), "observes[1] = 1 on a NULL slot"));
    o[1] = 2; CHECK(named(add(T, 4, s, o, px, lv, be), "observes[1] is neither 0 nor 1")); o[1] = 0;
    T[5] = nan; CHECK(named(add(T, 4, s, o, px, lv, be), "T_kf_w is not finite"));
    CHECK(named(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 1, T, 0, 0, nullptr, nullptr), "keyframe 1: T_kf_w is not finite")); T[5] = 1;
    CHECK(k == -5);
    CHECK(named(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 2, T, 0, 0, nullptr, nullptr), "keyframe 2"));
    CHECK(named(dsdtm_trackmap_keyframe_write(w.ctx, w.map, -1, T, 0, 0, nullptr, nullptr), "keyframe -1"));
    CHECK(named(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 0, nullptr, 2, 3, s, o), "keyframe 0: slots [2, 5) outside its 4 slots"));
    CHECK(named(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 0, nullptr, 0, 2, nullptr, o), "point_of_slot is NULL"));
    CHECK(named(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 0, nullptr, 0, 2, s, nullptr), "observes is NULL"));
    s[1] = 10; CHECK(named(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 1, nullptr, 2, 4, s, o), "keyframe 1: point_of_slot[1] = 10")); s[1] = -1;
    o[1] = 1; CHECK(named(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 1, nullptr, 2, 4, s, o), "keyframe 1: observes[1] = 1 on a NULL slot")); o[1] = 0;
    CHECK(dsdtm_trackmap_keyframe_write(w.ctx, w.map, 1, nullptr, 0, 0, nullptr, nullptr) == DSDTM_OK);      // nothing to write
    CHECK(named(dsdtm_trackmap_map_read(w.ctx, other.map, nullptr), "map"));
    CHECK(named(dsdtm_trackmap_map_read(w.ctx, w.map, nullptr), "out is NULL"));
    CHECK(named(dsdtm_trackmap_map_create(w.ctx, nullptr), "out is NULL"));
    // local
    const int n_local = 3, cap = 8, ocap = 8;
    std::vector<World::Out> out(3, World::Out(n_local, cap, ocap));
    dsdtm_trackmap_result res[3];
    dsdtm_trackmap_desc d[3];
    double Tc[3][12];
    auto reset = [&]() {
        fill_a5(res, sizeof res);
        for (int i = 0; i < 3; ++i) { memcpy(Tc[i], I12, sizeof I12); out[(size_t)i].fill(); d[i] = out[(size_t)i].desc(w.map, Tc[i]); }
    };
    dsdtm_localmap_params prm{n_local, 0};
    dsdtm_camera cam = CAM;
    auto loc = [&](const char* what) {
        const int rc = dsdtm_trackmap_local(w.ctx, &cam, &prm, 3, d, res);
        const bool ok = named(rc, what) && out[0].untouched() && out[1].untouched() && out[2].untouched() && all_a5(res, sizeof res);
        reset(); prm = dsdtm_localmap_params{n_local, 0}; cam = CAM;
        return ok;
    };
    reset();
    d[1].map = nullptr; CHECK(loc("desc 1: map is NULL"));
    d[2].map = other.map; CHECK(loc("desc 2: map is not a map of this context"));
    d[0].T_cur_w = nullptr; CHECK(loc("desc 0: T_cur_w is NULL"));
    d[1].kf = nullptr; CHECK(loc("desc 1: kf is NULL"));
    d[1].kf_dist = nullptr; CHECK(loc("desc 1: kf_dist is NULL"));
    d[2].point = nullptr; CHECK(loc("desc 2: point is NULL"));
    d[2].point_kf = nullptr; CHECK(loc("desc 2: point_kf is NULL"));
    d[2].mp_world = nullptr; CHECK(loc("desc 2: mp_world is NULL"));
    d[2].mp_found = nullptr; CHECK(loc("desc 2: mp_found is NULL"));
    d[2].mp_bad = nullptr; CHECK(loc("desc 2: mp_bad is NULL"));
    d[0].obs_offset = nullptr; CHECK(loc("desc 0: obs_offset is NULL"));
    d[0].obs_kf = nullptr; CHECK(loc("desc 0: obs_kf is NULL"));
    d[0].obs_px = nullptr; CHECK(loc("desc 0: obs_px is NULL"));
    d[0].obs_level = nullptr; CHECK(loc("desc 0: obs_level is NULL"));
    d[0].obs_bearing = nullptr; CHECK(loc("desc 0: obs_bearing is NULL"));
    d[2].point_capacity = -1; CHECK(loc("desc 2: point_capacity"));
    d[2].point_capacity = DSDTM_TRACKMAP_MAX_LOCAL_POINTS + 1; CHECK(loc("desc 2: point_capacity"));
    d[1].obs_capacity = -1; CHECK(loc("desc 1: obs_capacity"));
    Tc[1][11] = nan; CHECK(loc("desc 1: T_cur_w is not finite"));
    Tc[2][0] = -inf; CHECK(loc("desc 2: T_cur_w is not finite"));
    prm.n_local = 0; CHECK(loc("n_local"));
    prm.n_local = DSDTM_LOCALMAP_MAX_LOCAL + 1; CHECK(loc("n_local"));
    prm.boundary = -1; CHECK(loc("boundary"));
    cam.width = 0; CHECK(loc("camera size"));
    cam.height = -480; CHECK(loc("camera size"));
    d[1].obs_capacity = 2147483647; CHECK(loc("exceeds"));            // the call's memory limit: refused, nothing clipped
    CHECK(named(dsdtm_trackmap_local(w.ctx, nullptr, &prm, 3, d, res), "cam is NULL"));
    CHECK(named(dsdtm_trackmap_local(w.ctx, &cam, nullptr, 3, d, res), "params is NULL"));
    CHECK(named(dsdtm_trackmap_local(w.ctx, &cam, &prm, 3, nullptr, res), "descs is NULL"));
    CHECK(named(dsdtm_trackmap_local(w.ctx, &cam, &prm, 3, d, nullptr), "results is NULL"));
    CHECK(named(dsdtm_trackmap_local(w.ctx, &cam, &prm, -1, d, res), "n = -1"));
    CHECK(named(dsdtm_trackmap_local(w.ctx, &cam, &prm, DSDTM_LOCALMAP_MAX_DESCS + 1, d, res), "n = 1025"));
    CHECK(dsdtm_trackmap_local(w.ctx, &cam, &prm, 0, nullptr, nullptr) == DSDTM_OK);
    CHECK(dsdtm_trackmap_local(nullptr, &cam, &prm, 3, d, res) == DSDTM_ERR_INVALID && all_a5(res, sizeof res));
    CHECK(fake_hip_calls("hipMemcpyAsync") == copies);
    CHECK(fake_trackmap_update_launches() + fake_trackmap_flatten_launches() + fake_localmap_select_launches() == launches);
    // capacities of 0 with NULL lists are fine, and the descs of one map answer alike
    d[1].point_capacity = 0; d[1].point = nullptr; d[1].point_kf = nullptr; d[1].mp_world = nullptr; d[1].mp_found = nullptr; d[1].mp_bad = nullptr;
    d[1].obs_capacity = 0; d[1].obs_kf = nullptr; d[1].obs_px = nullptr; d[1].obs_level = nullptr; d[1].obs_bearing = nullptr;
    CHECK(dsdtm_trackmap_local(w.ctx, &cam, &prm, 3, d, res) == DSDTM_OK);
    CHECK(res[0].n_points == res[1].n_points && res[1].overflow_points == (res[1].n_points > 0) && res[1].n_obs == 0 && memcmp(&res[0], &res[2], sizeof res[0]) == 0);
    CHECK(out[0].same(out[2]) && !out[0].untouched() && out[1].oo[0] == 0);
    CHECK(w.agrees() && other.agrees());
    other.close(); w.close();
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// a HIP call that fails, at every call site of every entry: an error, the map as it was, the outputs untouched, nothing pending,
// nothing leaked; the context stays usable
static bool hip_failures() {
    const char* apis[] = {"hipMemcpyAsync", "hipStreamSynchronize", "hipMalloc", "hipHostMalloc", "hipSetDevice", "launch", "select launch"};
    for (int entry = 0; entry < 7; ++entry)
        for (const char* api : apis)
            for (long nth = 1; nth <= 7; ++nth) {
                World w;
                CHECK(w.open());
                if (entry != 0) CHECK(w.points(dsdtm::LM_INITIAL_POINTS - 2) && w.keyframe(300));      // the next update grows arrays
                if (entry >= 4) CHECK(w.agrees());                                                 // (and the stream is idle)
                const bool launch = !strcmp(api, "launch"), select = !strcmp(api, "select launch");
                if (launch) fake_trackmap_fail(nth); else if (select) fake_localmap_fail(nth); else fake_hip_fail(api, nth);
                int rc = DSDTM_OK;
                const double x[12] = {0.1, 0.1, 2.0, 0.2, 0.1, 2.0, 0.3, 0.1, 2.0, 0.4, 0.1, 2.0};
                const int32_t f4[4] = {3, 1, 4, 1}, idx[2] = {0, 5}, val[2] = {60, 61};
                const Slots c = w.draw(entry == 3 ? 20 : 300);
                double T[12];
                memcpy(T, I12, sizeof T);
                T[7] = 0.5;
                int k = -5;
                World::Out out(2, 4, 6);
                dsdtm_trackmap_result res;
                fill_a5(&res, sizeof res);
                dsdtm_trackmap_image im{};
                if (entry == 0 || entry == 1) rc = dsdtm_trackmap_points_write(w.ctx, w.map, w.m.P(), 4, x, nullptr, f4);
                else if (entry == 2) rc = dsdtm_trackmap_keyframe_add(w.ctx, w.map, T, 300, c.s.data(), c.o.data(), c.px.data(), c.level.data(), c.bearing.data(), &k);
                else if (entry == 3) rc = dsdtm_trackmap_keyframe_write(w.ctx, w.map, 0, T, 30, 20, c.s.data(), c.o.data());
                else if (entry == 4) rc = dsdtm_trackmap_found_write(w.ctx, w.map, 2, idx, val);
                else if (entry == 5) rc = dsdtm_trackmap_map_read(w.ctx, w.map, &im);      // (sizing call: no HIP call on the way; agrees() below reads in full)
                else {
                    dsdtm_localmap_params prm{2, 0};
                    dsdtm_trackmap_desc d = out.desc(w.map, I12);
                    rc = dsdtm_trackmap_local(w.ctx, &CAM, &prm, 1, &d, &res);
                }
                fake_trackmap_fail(0); fake_localmap_fail(0);
                if (!launch && !select) fake_hip_fail(api, 0);
                if (rc == DSDTM_OK) {            // (fewer than nth calls of this api on the way)
                    if (entry <= 1) { w.m.p.insert(w.m.p.end(), x, x + 12); w.m.bad.insert(w.m.bad.end(), 4, 0); w.m.found.insert(w.m.found.end(), f4, f4 + 4); }
                    if (entry == 2) {
                        CHECK(k == w.m.K());
                        w.m.off.push_back((int64_t)w.m.slots.size()); w.m.ns.push_back(300); w.m.T.insert(w.m.T.end(), T, T + 12);
                        w.m.slots.insert(w.m.slots.end(), c.s.begin(), c.s.end()); w.m.observes.insert(w.m.observes.end(), c.o.begin(), c.o.end());
                        w.m.px.insert(w.m.px.end(), c.px.begin(), c.px.end()); w.m.level.insert(w.m.level.end(), c.level.begin(), c.level.end());
                        w.m.bearing.insert(w.m.bearing.end(), c.bearing.begin(), c.bearing.end());
                    }
                    if (entry == 3) { memcpy(&w.m.T[0], T, sizeof T); std::copy(c.s.begin(), c.s.end(), w.m.slots.begin() + 30); std::copy(c.o.begin(), c.o.end(), w.m.observes.begin() + 30); }
                    if (entry == 4) { w.m.found[0] = 60; w.m.found[5] = 61; }
                } else {
                    CHECK(rc == DSDTM_ERR_HIP && strlen(dsdtm_trackmap_last_error(w.ctx)) > 0 && k == -5);
                    CHECK(out.untouched() && all_a5(&res, sizeof res));
                }
                CHECK(w.agrees());               // the map as it was (or as updated), and the context usable
                CHECK(w.points(5) && w.keyframe(9) && w.agrees());
                w.close();
                CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0);
            }
    // map_read's own copies and wait failing: the image's arrays may be partly written, the map is as it was
    for (long nth = 1; nth <= 7; ++nth)
        for (const char* api : {"hipMemcpyAsync", "hipStreamSynchronize", "hipSetDevice"}) {
            World w;
            CHECK(w.open() && w.points(20) && w.keyframe(12) && w.agrees());
            fake_hip_fail(api, nth);
            const bool ok = w.agrees();
            fake_hip_fail(api, 0);
            CHECK(ok || strlen(dsdtm_trackmap_last_error(w.ctx)) > 0);
            CHECK(w.agrees() && w.points(3) && w.agrees());
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
    Slots c = w.draw(DSDTM_LOCALMAP_MAX_SLOTS);
    int k = -1;
    CHECK(dsdtm_trackmap_keyframe_add(w.ctx, w.map, I12, DSDTM_LOCALMAP_MAX_SLOTS, c.s.data(), c.o.data(), c.px.data(), c.level.data(), c.bearing.data(), &k) == DSDTM_OK && k == 0);
    w.m.off.push_back(0); w.m.ns.push_back(DSDTM_LOCALMAP_MAX_SLOTS); w.m.T.assign(I12, I12 + 12);
    w.m.slots = c.s; w.m.observes = c.o; w.m.px = c.px; w.m.level = c.level; w.m.bearing = c.bearing;
    CHECK(w.agrees(DSDTM_LOCALMAP_MAX_LOCAL, DSDTM_TRACKMAP_MAX_LOCAL_POINTS, 5000));
    // 1024 descs of one map in one call: one selection, one flatten
    const int n = DSDTM_LOCALMAP_MAX_DESCS, n_local = 2;
    std::vector<World::Out> out;
    std::vector<dsdtm_trackmap_desc> d((size_t)n);
    std::vector<dsdtm_trackmap_result> res((size_t)n);
    std::vector<double> T((size_t)n * 12);
    out.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        memcpy(&T[12 * (size_t)i], I12, sizeof I12);
        T[12 * (size_t)i + 3] = 0.001 * i;
        out.emplace_back(n_local, i % 4, i % 3);
        d[(size_t)i] = out.back().desc(w.map, &T[12 * (size_t)i]);
    }
    dsdtm_localmap_params prm{n_local, 0};
    const long l0 = fake_trackmap_flatten_launches(), s0 = fake_localmap_select_launches();
    CHECK(dsdtm_trackmap_local(w.ctx, &CAM, &prm, n, d.data(), res.data()) == DSDTM_OK);
    CHECK(fake_trackmap_flatten_launches() == l0 + 1 && fake_localmap_select_launches() == s0 + 1);
    for (int i = 0; i < n; ++i) {
        const dsdtm_trackmap_result& r = res[(size_t)i];
        CHECK(r.n_close == 1 && r.n_kf == 1 && r.overflow_points == 1 && r.n_points == res[0].n_points && out[(size_t)i].kd[0] == std::fabs(0.001 * i));
        CHECK(out[(size_t)i].oo[(size_t)(i % 4)] == r.n_obs && r.overflow_obs == (r.n_obs > i % 3));
    }
    // a call just under the memory limit's refusal, and one over it
    World::Out one(n_local, 4, 4);
    dsdtm_trackmap_desc big = one.desc(w.map, I12);
    big.obs_capacity = (int32_t)(DSDTM_TRACKMAP_MAX_CALL_BYTES / 48 + 1);
    CHECK(named_err(w.ctx, dsdtm_trackmap_local(w.ctx, &CAM, &prm, 1, &big, res.data()), "exceeds") && one.untouched());
    w.close();
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_trackmap", dsdtm_trackmap_create, dsdtm_trackmap_destroy, dsdtm_trackmap_last_error);
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"updates_and_growth", updates_and_growth}, {"found_write_refusals", found_write_refusals},
                                                      {"validation", validation}, {"hip_failures", hip_failures}, {"limits", limits},
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
