// dsdtm_newkf_make_batch against the fake HIP runtime of tests/fake_hip (unmodified): the host side of libdsdtm_amd_newkf.so
// (dsdtm_amd/csrc/newkf_api.cpp) — the context, the checks, the one rule that decides whether a caller's array is staged or read in
// place, the block's layout, the one upload / one launch / one read-back, every failure path — under ASan/UBSan/LSan. The launch is the
// fake of tests/fake_hip_newkf/fake_newkf.cpp, which answers with create_keyframe_host on what it finds in "device" memory. Test
// infrastructure (tests/test_newkf_cpu.py); nothing here is part of the product.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../dsdtm_amd/host/dsdtm_newkf_host.hpp"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_newkf.h"

static const dsdtm_camera CAM{525.f, 525.5f, 87.25f, 49.5f, 525.f, 176, 100};
static dsdtm_newkf_params params() {
    dsdtm_newkf_params p{};
    p.width = 176; p.height = 100; p.cell_size = 12; p.grid_cols = 15; p.grid_rows = 9; p.max_fts = 60; p.min_dist = 6; p.score_floor = 20.f;
    return p;
}
enum Mem { PAGEABLE, PINNED, DEVICE };

// an array of the caller in one of the three kinds of memory (in the fake all three are readable by the host)
template <class T>
struct Arr {
    std::vector<T> v; T* p = nullptr; Mem mem = PAGEABLE;
    void init(const std::vector<T>& src, Mem m) {
        release(); mem = m; v = src;
        if (m == PAGEABLE) { p = v.data(); return; }
        void* q = nullptr;
        if ((m == PINNED ? hipHostMalloc(&q, src.size() * sizeof(T), 0) : hipMalloc(&q, src.size() * sizeof(T))) != hipSuccess) { p = nullptr; return; }
        p = (T*)q; memcpy(p, src.data(), src.size() * sizeof(T));
    }
    void release() { if (p && mem == PINNED) (void)hipHostFree(p); if (p && mem == DEVICE) (void)hipFree(p); p = nullptr; }
    ~Arr() { release(); }
};

struct Tracker {
    dsdtm_newkf_params prm;
    Arr<float> score; Arr<int32_t> cx, cy, cl; Arr<uint16_t> depth; Arr<uint8_t> dyn;
    std::vector<float> px; std::vector<int32_t> level, point; std::vector<double> bearing, T; std::vector<uint8_t> has, initial;
    int depth_stride = 0;
    dsdtm_newkf_desc d{};
    // the outputs
    std::vector<int32_t> o_pos, o_level; std::vector<uint8_t> o_obs, o_bad; std::vector<float> o_px, o_depth; std::vector<double> o_bearing, o_pw;
    dsdtm_newkf_result r{};
    void init(int id, const dsdtm_newkf_params& p, int ne, Mem cells, Mem dep, Mem mask, bool with_dyn, int pad = 0) {
        prm = p;
        const size_t G = (size_t)p.grid_cols * p.grid_rows, W = (size_t)p.width, H = (size_t)p.height;
        std::vector<float> s(G); std::vector<int32_t> x(G), y(G), l(G);
        for (size_t k = 0; k < G; ++k) {
            s[k] = (float)(((k * 7 + (size_t)id * 3) % 11) * 5);                          // 0, 5, .. 50: ties; 20 does not pass
            x[k] = (int32_t)std::min(W - 1, (k % (size_t)p.grid_cols) * (size_t)p.cell_size + (k * 5 + (size_t)id) % (size_t)std::max(1, p.cell_size));
            y[k] = (int32_t)std::min(H - 1, (k / (size_t)p.grid_cols) * (size_t)p.cell_size + (k * 3 + (size_t)id) % (size_t)std::max(1, p.cell_size));
            l[k] = (int32_t)(k % 3);
        }
        score.init(s, cells); cx.init(x, cells); cy.init(y, cells); cl.init(l, cells);
        depth_stride = p.width + pad;
        std::vector<uint16_t> dp((size_t)depth_stride * H);
        for (size_t i = 0; i < dp.size(); ++i) dp[i] = (uint16_t)((i * 2654435761u + (size_t)id) % 7 == 0 ? 0 : 500 + (i * 37 + (size_t)id) % 30000);
        depth.init(dp, dep);
        std::vector<uint8_t> dm(W * H);
        for (size_t i = 0; i < dm.size(); ++i) dm[i] = (uint8_t)((i * 31 + (size_t)id) % 5 == 0 ? 255 : 200);
        dyn.init(dm, mask);
        px.resize(2 * (size_t)ne); level.resize((size_t)ne); point.resize((size_t)ne); bearing.resize(3 * (size_t)ne); has.resize((size_t)ne); initial.resize((size_t)ne);
        for (int k = 0; k < ne; ++k) {
            px[2 * k] = (float)((k * 37 + id * 11) % p.width) + 0.5f * (float)(k % 2); px[2 * k + 1] = (float)((k * 23 + id * 7) % p.height) + 0.25f;
            level[k] = k % 4; initial[k] = (uint8_t)(k % 3 == 0); has[k] = (uint8_t)(k % 3 != 1); point[k] = has[k] ? k : -1;
            bearing[3 * k] = 0.6; bearing[3 * k + 1] = 0.0; bearing[3 * k + 2] = 0.8;
        }
        T = {0.8, -0.6, 0, 0.5 + id, 0.6, 0.8, 0, -0.25, 0, 0, 1, 0.125 * id};
        d = dsdtm_newkf_desc{};
        d.cell_score = score.p; d.cell_x = cx.p; d.cell_y = cy.p; d.cell_level = cl.p;
        d.n_existing = ne; d.first_point_index = 100 * id;
        d.px_xy = px.data(); d.level = level.data(); d.bearing = bearing.data(); d.has_point = has.data(); d.initial = initial.data(); d.point_index = point.data();
        d.depth = depth.p; d.depth_stride = depth_stride; d.depth_scale = 4096.0f;
        d.dyn_mask = with_dyn ? dyn.p : nullptr; d.dyn_stride = p.width;
        d.T_c2w = T.data();
        capacities(ne + (int)G, ne + (int)G);
    }
    void capacities(int slots, int points) {
        d.slot_capacity = slots; d.point_capacity = points; d.bad_capacity = points;
        const size_t S = (size_t)std::max(slots, 1), P = (size_t)std::max(points, 1);
        o_pos.resize(S); o_level.resize(S); o_obs.resize(S); o_px.resize(2 * S); o_depth.resize(S); o_bearing.resize(3 * S); o_pw.resize(3 * P); o_bad.resize(P);
        r.point_of_slot = o_pos.data(); r.observes = o_obs.data(); r.px_xy = o_px.data(); r.level = o_level.data(); r.bearing = o_bearing.data();
        r.depth_of_slot = o_depth.data(); r.new_p_world = o_pw.data(); r.new_bad = o_bad.data();
        prefill();
    }
    void prefill() {
        fill_a5(&r, 16);
        fill_a5(o_pos.data(), o_pos.size() * 4); fill_a5(o_level.data(), o_level.size() * 4); fill_a5(o_obs.data(), o_obs.size());
        fill_a5(o_px.data(), o_px.size() * 4); fill_a5(o_depth.data(), o_depth.size() * 4); fill_a5(o_bearing.data(), o_bearing.size() * 8);
        fill_a5(o_pw.data(), o_pw.size() * 8); fill_a5(o_bad.data(), o_bad.size());
    }
    bool arrays_untouched() const {
        return all_a5(o_pos.data(), o_pos.size() * 4) && all_a5(o_level.data(), o_level.size() * 4) && all_a5(o_obs.data(), o_obs.size()) &&
               all_a5(o_px.data(), o_px.size() * 4) && all_a5(o_depth.data(), o_depth.size() * 4) && all_a5(o_bearing.data(), o_bearing.size() * 8) &&
               all_a5(o_pw.data(), o_pw.size() * 8) && all_a5(o_bad.data(), o_bad.size());
    }
    bool untouched() const { return all_a5(&r, 16) && arrays_untouched(); }
    // the result equals create_keyframe_host on the caller's own desc, and nothing behind the counts was written
    bool answered(const dsdtm_newkf_result& got) const {
        const DSDTM::NewKeyframeHost w = DSDTM::create_keyframe_host(CAM, prm, d);
        CHECK(got.n_new == w.n_new && got.n_slots == w.n_slots && got.n_new_points == w.n_new_points && got.overflow == 0);
        const size_t S = (size_t)w.n_slots, P = (size_t)w.n_new_points;
        CHECK(S <= o_pos.size() && P * 3 <= o_pw.size());
        CHECK(!S || (!memcmp(got.point_of_slot, w.point_of_slot.data(), S * 4) && !memcmp(got.observes, w.observes.data(), S) &&
                     !memcmp(got.px_xy, w.px_xy.data(), S * 8) && !memcmp(got.level, w.level.data(), S * 4) &&
                     !memcmp(got.bearing, w.bearing.data(), S * 24) && !memcmp(got.depth_of_slot, w.depth_of_slot.data(), S * 4)));
        CHECK(!P || !memcmp(got.new_p_world, w.new_p_world.data(), P * 24));
        for (size_t i = 0; i < P; ++i) CHECK(got.new_bad[i] == 0);
        if (got.point_of_slot == o_pos.data()) {
            CHECK(all_a5(o_pos.data() + S, (o_pos.size() - S) * 4) && all_a5(o_pw.data() + 3 * P, (o_pw.size() - 3 * P) * 8) && all_a5(o_bad.data() + P, o_bad.size() - P));
        }
        return true;
    }
};

struct Batch {
    std::vector<Tracker> t;
    std::vector<dsdtm_newkf_desc> d;
    std::vector<dsdtm_newkf_result> r;
    dsdtm_newkf_params p = params();
    explicit Batch(size_t n) : t(n) {}
    void refresh() { d.clear(); r.clear(); for (auto& x : t) { d.push_back(x.d); r.push_back(x.r); } }
    void prefill() { for (auto& x : t) x.prefill(); refresh(); }
    int run(dsdtm_newkf_ctx* ctx) { return dsdtm_newkf_make_batch(ctx, &CAM, &p, (int)d.size(), d.data(), r.data()); }
    bool untouched() const {
        for (size_t i = 0; i < t.size(); ++i) if (!all_a5(&r[i], 16) || !t[i].arrays_untouched()) return false;
        return true;
    }
    bool answered() const { for (size_t i = 0; i < t.size(); ++i) if (!t[i].answered(r[i])) return false; return true; }
};

static void standard(Batch& b) {
    const dsdtm_newkf_params p = b.p;
    b.t[0].init(0, p, 0, PAGEABLE, PAGEABLE, PAGEABLE, true);           // an empty frame: the mask is ignored
    b.t[1].init(1, p, 17, PINNED, PINNED, PINNED, true);
    b.t[2].init(2, p, 25, DEVICE, DEVICE, DEVICE, true);
    b.t[3].init(3, p, 70, PAGEABLE, DEVICE, PAGEABLE, false);           // K1
    b.t[4].init(4, p, 9, DEVICE, PAGEABLE, PINNED, true, /*pad=*/5);    // a padded depth image in pageable memory: staged row by row
    b.refresh();
}

// every kind of memory for every array: a pageable array is staged (the kernel is given an address inside the block), a pinned or a
// device array is read in place (the kernel is given the caller's address); the answers are create_keyframe_host's; one launch
static bool answers_and_memory_kinds() {
    dsdtm_newkf_ctx* ctx = nullptr;
    CHECK(dsdtm_newkf_create(0, &ctx) == DSDTM_OK);
    {
        Batch b(5);
        standard(b);
        const long l0 = fake_newkf_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
        CHECK(b.run(ctx) == DSDTM_OK && b.answered());
        CHECK(fake_newkf_launches() == l0 + 1 && fake_hip_calls("hipMemcpyAsync") == c0 + 2 && fake_hip_pending() == 0);
        for (int t = 0; t < 5; ++t) {
            const Tracker& k = b.t[(size_t)t];
            CHECK((fake_newkf_seen(t, 0) == k.score.p) == (k.score.mem != PAGEABLE) && (fake_newkf_seen(t, 3) == k.cx.p) == (k.cx.mem != PAGEABLE));
            CHECK((fake_newkf_seen(t, 1) == k.depth.p) == (k.depth.mem != PAGEABLE));
            if (k.d.dyn_mask) CHECK((fake_newkf_seen(t, 2) == k.dyn.p) == (k.dyn.mem != PAGEABLE));
            else CHECK(fake_newkf_seen(t, 2) == nullptr);
        }
        CHECK(b.r[3].n_new == 0 && b.r[3].n_slots == 70 && b.r[0].n_new > 5 && b.r[4].n_new_points > 5);
        // the single entry is the batch entry with n = 1, and gives the batch's answer
        for (size_t t = 0; t < 5; ++t) {
            b.t[t].prefill();
            dsdtm_newkf_result one = b.t[t].r;
            CHECK(dsdtm_newkf_make(ctx, &CAM, &b.p, &b.t[t].d, &one) == DSDTM_OK && b.t[t].answered(one));
        }
    }
    dsdtm_newkf_destroy(ctx);
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// every refusal names the tracker and the field, enqueues nothing and leaves the results of ALL trackers untouched
static bool refusals() {
    dsdtm_newkf_ctx* ctx = nullptr;
    CHECK(dsdtm_newkf_create(0, &ctx) == DSDTM_OK);
    {
        Batch b(5);
        standard(b);
        CHECK(b.run(ctx) == DSDTM_OK && b.answered());
        b.prefill();
        const long l0 = fake_newkf_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
        auto invalid = [&](const char* what) {
            const int rc = b.run(ctx);
            if (rc != DSDTM_ERR_INVALID || !b.untouched() || !strstr(dsdtm_newkf_last_error(ctx), what)) {
                std::fprintf(stderr, "expected INVALID naming '%s': rc %d, error '%s'\n", what, rc, dsdtm_newkf_last_error(ctx));
                return false;
            }
            return true;
        };
        const float nanf_ = std::numeric_limits<float>::quiet_NaN();
        const double inf = std::numeric_limits<double>::infinity();
        b.t[2].T[7] = inf; CHECK(invalid("tracker 2: T_c2w is not finite")); b.t[2].T[7] = -0.25;
        b.t[1].px[9] = nanf_; CHECK(invalid("tracker 1: px_xy is not finite (entry 4)")); b.t[1].px[9] = 3.25f;
        b.t[2].level[24] = 16; CHECK(invalid("tracker 2: level outside 0..15 (entry 24)")); b.t[2].level[24] = -1; CHECK(invalid("tracker 2: level")); b.t[2].level[24] = 0;
        b.t[4].point[3] = -1; CHECK(b.t[4].initial[3] == 1 && invalid("tracker 4: initial feature with point_index < 0 (entry 3)")); b.t[4].point[3] = 3;
        // cells the host can read: pageable and pinned ones; the same in device memory is the kernel's to skip
        b.t[0].cx.p[7] = -1; CHECK(invalid("tracker 0: cell_x is negative (entry 7)")); b.t[0].cx.p[7] = 3;
        b.t[1].cy.p[134] = -5; CHECK(invalid("tracker 1: cell_y is negative (entry 134)")); b.t[1].cy.p[134] = 3;
        b.t[0].cl.p[0] = -1; CHECK(invalid("tracker 0: cell_level is negative (entry 0)")); b.t[0].cl.p[0] = 0;
        b.d[1].slot_capacity = 16; CHECK(invalid("tracker 1: slot_capacity below n_existing")); b.refresh();
        b.d[1].point_capacity = -1; CHECK(invalid("tracker 1: point_capacity")); b.refresh();
        b.d[3].n_existing = DSDTM_NEWKF_MAX_EXISTING + 1; CHECK(invalid("tracker 3: n_existing")); b.refresh();
        b.d[3].n_existing = -1; CHECK(invalid("tracker 3: n_existing")); b.refresh();
        b.d[2].depth = nullptr; CHECK(invalid("tracker 2: depth is NULL")); b.refresh();
        b.d[2].depth_stride = 175; CHECK(invalid("tracker 2: depth_stride")); b.refresh();
        b.d[2].depth_scale = 0.0f; CHECK(invalid("tracker 2: depth_scale")); b.refresh();
        b.d[2].dyn_stride = 100; CHECK(invalid("tracker 2: dyn_stride")); b.refresh();
        b.d[4].cell_level = nullptr; CHECK(invalid("tracker 4: a cell array is NULL")); b.refresh();
        b.d[4].has_point = nullptr; CHECK(invalid("tracker 4: an existing-feature array is NULL")); b.refresh();
        b.d[4].T_c2w = nullptr; CHECK(invalid("tracker 4: T_c2w is NULL")); b.refresh();
        b.d[4].first_point_index = -1; CHECK(invalid("tracker 4: first_point_index")); b.refresh();
        b.r[0].bearing = nullptr; CHECK(b.run(ctx) == DSDTM_ERR_INVALID && strstr(dsdtm_newkf_last_error(ctx), "tracker 0: a slot column")); b.refresh();
        b.r[0].new_p_world = nullptr; CHECK(b.run(ctx) == DSDTM_ERR_INVALID && strstr(dsdtm_newkf_last_error(ctx), "tracker 0: new_p_world")); b.refresh();
        // the shared arguments
        dsdtm_newkf_params keep = b.p;
        b.p.cell_size = 128; CHECK(invalid("cell_size")); b.p = keep;
        b.p.min_dist = -1; CHECK(invalid("min_dist")); b.p = keep;
        b.p.grid_cols = 64; b.p.grid_rows = 65; CHECK(invalid("grid_cols x grid_rows")); b.p = keep;
        b.p.width = 0; CHECK(invalid("width")); b.p = keep;
        b.p.height = DSDTM_NEWKF_MAX_SIDE + 1; CHECK(invalid("height")); b.p = keep;
        b.p.score_floor = nanf_; CHECK(invalid("score_floor")); b.p.score_floor = -1.0f; CHECK(invalid("score_floor")); b.p = keep;
        b.p.max_fts = -1; CHECK(invalid("max_fts")); b.p = keep;
        CHECK(dsdtm_newkf_make_batch(ctx, &CAM, &b.p, 0, b.d.data(), b.r.data()) == DSDTM_ERR_INVALID && b.untouched());
        CHECK(dsdtm_newkf_make_batch(ctx, &CAM, &b.p, DSDTM_NEWKF_MAX_TRACKERS + 1, b.d.data(), b.r.data()) == DSDTM_ERR_INVALID);
        CHECK(dsdtm_newkf_make_batch(ctx, nullptr, &b.p, 5, b.d.data(), b.r.data()) == DSDTM_ERR_INVALID);
        CHECK(dsdtm_newkf_make_batch(ctx, &CAM, nullptr, 5, b.d.data(), b.r.data()) == DSDTM_ERR_INVALID);
        CHECK(dsdtm_newkf_make_batch(ctx, &CAM, &b.p, 5, nullptr, b.r.data()) == DSDTM_ERR_INVALID);
        CHECK(dsdtm_newkf_make_batch(ctx, &CAM, &b.p, 5, b.d.data(), nullptr) == DSDTM_ERR_INVALID);
        CHECK(dsdtm_newkf_make_batch(nullptr, &CAM, &b.p, 5, b.d.data(), b.r.data()) == DSDTM_ERR_INVALID);
        dsdtm_camera cam = CAM; cam.fx = 0.0f;
        CHECK(dsdtm_newkf_make_batch(ctx, &cam, &b.p, 5, b.d.data(), b.r.data()) == DSDTM_ERR_INVALID && b.untouched());
        CHECK(fake_newkf_launches() == l0 && fake_hip_calls("hipMemcpyAsync") == c0 && fake_hip_pending() == 0);      // nothing was enqueued
        // a negative pixel among DEVICE cells passes the host (tracker 2's cells are in device memory)
        b.t[2].cx.p[5] = -3;
        CHECK(b.run(ctx) == DSDTM_OK && b.answered());
        b.t[2].cx.p[5] = 3;
        // existing-feature arrays may be NULL when there is no existing feature
        b.d[0].px_xy = nullptr; b.d[0].has_point = nullptr; b.d[0].initial = nullptr; b.d[0].level = nullptr; b.d[0].bearing = nullptr; b.d[0].point_index = nullptr;
        b.prefill(); b.d[0].px_xy = nullptr; b.d[0].has_point = nullptr;
        CHECK(b.run(ctx) == DSDTM_OK && b.answered());
    }
    dsdtm_newkf_destroy(ctx);
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// the upload, the launch, the read-back and the wait each fail once, the device view of a pinned array cannot be had, a staging block
// that must grow cannot be had: an error, the results untouched, nothing pending, nothing leaked; the context stays usable
static bool hip_failures() {
    dsdtm_newkf_ctx* ctx = nullptr;
    CHECK(dsdtm_newkf_create(0, &ctx) == DSDTM_OK);
    {
        Batch b(5);
        standard(b);
        CHECK(b.run(ctx) == DSDTM_OK && b.answered());
        const size_t live0 = fake_hip_live_allocations();
        for (const char* api : {"hipMemcpyAsync", "hipStreamSynchronize"})
            for (long nth = 1; nth <= 2; ++nth) {            // 1: the upload / the launch's drain; 2: the read-back / the wait
                b.prefill();
                fake_hip_fail(api, nth);
                const int rc = b.run(ctx);
                fake_hip_fail(api, 0);
                CHECK(rc == DSDTM_ERR_HIP && b.untouched() && fake_hip_pending() == 0 && strlen(dsdtm_newkf_last_error(ctx)) > 0);
                b.prefill();
                CHECK(b.run(ctx) == DSDTM_OK && b.answered());
            }
        b.prefill();
        fake_newkf_fail(1);
        CHECK(b.run(ctx) == DSDTM_ERR_HIP && b.untouched() && fake_hip_pending() == 0);
        fake_newkf_fail(0);
        for (long nth = 1; nth <= 3; ++nth) {               // (the batch has pinned arrays in trackers 1 and 4)
            b.prefill();
            fake_hip_fail("hipHostGetDevicePointer", nth);
            const int rc = b.run(ctx);
            fake_hip_fail("hipHostGetDevicePointer", 0);
            CHECK(rc == DSDTM_ERR_HIP && b.untouched() && fake_hip_pending() == 0);
        }
        b.prefill();
        fake_hip_fail("hipSetDevice", 1);
        CHECK(b.run(ctx) == DSDTM_ERR_HIP && b.untouched());
        fake_hip_fail("hipSetDevice", 0);
        b.prefill();
        CHECK(b.run(ctx) == DSDTM_OK && b.answered());
        CHECK(fake_hip_live_allocations() == live0);
        dsdtm_newkf_destroy(ctx);
        // a fresh context whose staging block cannot be had: pinned, then device
        for (const char* api : {"hipHostMalloc", "hipMalloc"}) {
            CHECK(dsdtm_newkf_create(0, &ctx) == DSDTM_OK);
            for (long nth = 1; nth <= 2; ++nth) {
                b.prefill();
                fake_hip_fail(api, nth);
                const int rc = b.run(ctx);
                fake_hip_fail(api, 0);
                if (rc == DSDTM_OK) { CHECK(b.answered()); continue; }      // (fewer than nth calls of this api)
                CHECK(rc == DSDTM_ERR_HIP && b.untouched() && fake_hip_pending() == 0);
                b.prefill();
                CHECK(b.run(ctx) == DSDTM_OK && b.answered());
            }
            dsdtm_newkf_destroy(ctx);
        }
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// a capacity that does not fit: overflow is reported with the right counts, nothing of that tracker is written, the others are answered
static bool overflow() {
    dsdtm_newkf_ctx* ctx = nullptr;
    CHECK(dsdtm_newkf_create(0, &ctx) == DSDTM_OK);
    {
        Batch b(5);
        standard(b);
        CHECK(b.run(ctx) == DSDTM_OK && b.answered());
        const dsdtm_newkf_result full1 = b.r[1], full2 = b.r[2], full4 = b.r[4];
        CHECK(full1.n_new > 2 && full2.n_new_points > 2 && full4.n_new_points > 2);
        b.t[1].capacities(full1.n_slots - 1, full1.n_slots);                   // one slot short
        b.t[2].capacities(full2.n_slots, full2.n_new_points - 1);              // one point short
        b.t[4].capacities(full4.n_slots, full4.n_new_points); b.t[4].d.bad_capacity = full4.n_new_points - 1;      // new_bad one short
        b.t[0].prefill(); b.t[3].prefill();
        b.refresh();
        CHECK(b.run(ctx) == DSDTM_OK);
        for (size_t t : {(size_t)1, (size_t)2, (size_t)4}) {
            const dsdtm_newkf_result& w = t == 1 ? full1 : t == 2 ? full2 : full4;
            CHECK(b.r[t].overflow == 1 && b.r[t].n_new == w.n_new && b.r[t].n_slots == w.n_slots && b.r[t].n_new_points == w.n_new_points);
            CHECK(b.t[t].arrays_untouched());
        }
        CHECK(b.t[0].answered(b.r[0]) && b.t[3].answered(b.r[3]));
        // exactly enough is enough
        b.t[1].capacities(full1.n_slots, full1.n_new_points); b.t[2].capacities(full2.n_slots, full2.n_new_points);
        b.t[4].capacities(full4.n_slots, full4.n_new_points);
        b.prefill();
        CHECK(b.run(ctx) == DSDTM_OK && b.answered());
    }
    dsdtm_newkf_destroy(ctx);
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// n, G and the radii at their limits
static bool limits() {
    dsdtm_newkf_ctx* ctx = nullptr;
    CHECK(dsdtm_newkf_create(0, &ctx) == DSDTM_OK);
    {
        Batch b(DSDTM_NEWKF_MAX_TRACKERS);
        b.p.width = 40; b.p.height = 30; b.p.cell_size = 10; b.p.grid_cols = 4; b.p.grid_rows = 3; b.p.max_fts = 12; b.p.min_dist = 3;
        for (int i = 0; i < DSDTM_NEWKF_MAX_TRACKERS; ++i) b.t[(size_t)i].init(i, b.p, i % 14, (Mem)(i % 3), (Mem)((i / 3) % 3), (Mem)((i / 9) % 3), i % 2 == 0);
        b.refresh();
        const long l0 = fake_newkf_launches();
        dsdtm_camera cam = CAM;
        CHECK(dsdtm_newkf_make_batch(ctx, &cam, &b.p, (int)b.d.size(), b.d.data(), b.r.data()) == DSDTM_OK && fake_newkf_launches() == l0 + 1);      // ONE launch for 1024 trackers
        for (size_t i = 0; i < b.t.size(); ++i) CHECK(b.t[i].answered(b.r[i]));
    }
    {
        Batch b(1);
        b.p.width = 1024; b.p.height = 1024; b.p.cell_size = 127; b.p.min_dist = 127; b.p.grid_cols = 64; b.p.grid_rows = 64; b.p.max_fts = 100000;
        b.t[0].init(1, b.p, DSDTM_NEWKF_MAX_EXISTING, PAGEABLE, PINNED, DEVICE, true);
        b.refresh();
        CHECK(b.run(ctx) == DSDTM_OK && b.answered());
    }
    dsdtm_newkf_destroy(ctx);
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_newkf", dsdtm_newkf_create, dsdtm_newkf_destroy, dsdtm_newkf_last_error);
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"answers_and_memory_kinds", answers_and_memory_kinds}, {"refusals", refusals},
                                                      {"hip_failures", hip_failures}, {"overflow", overflow}, {"limits", limits},
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
