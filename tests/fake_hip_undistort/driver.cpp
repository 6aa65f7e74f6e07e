// libdsdtm_amd_undistort.so's host side (dsdtm_amd/csrc/undistort_api.cpp) against the fake HIP runtime of tests/fake_hip (unmodified): the
// context, the map, the checks, the three memory kinds of a source and the two of a destination, the one upload / one launch / one
// read-back / one wait, every refusal and every HIP call failing in turn — as a stand-alone program under ASan/UBSan/LSan. The launches
// are the fakes of tests/fake_hip_undistort/fake_undistort.cpp. Test infrastructure (tests/test_undistort_cpu.py); nothing here is part
// of the product.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_undistort.h"
#include "../../dsdtm_amd/host/dsdtm_undistort_host.hpp"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_undistort.h"

enum Mem { PAGEABLE, PINNED, DEVICE };
static const float DIST_A[5] = {0.3f, -0.1f, 0.01f, -0.02f, 0.05f}, DIST_B[5] = {-0.2f, 0.0f, 0.0f, 0.01f, 0.0f};

static dsdtm_camera camera(int w, int h) {
    dsdtm_camera c{};
    c.fx = c.fy = (float)w * 0.9f; c.cx = (float)(w - 1) / 2; c.cy = (float)(h - 1) / 2; c.f = c.fx; c.width = w; c.height = h;
    return c;
}

// a buffer of exactly `bytes` in one of the three memories (an access outside it is ASan's)
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

// one frame: sources filled from a pattern, destinations prefilled with 0xA5; strides wider than the width and all different
struct Frame {
    int w = 0, h = 0, gs = 0, gd = 0, zs = 0, zd = 0;
    bool depth = false;
    Buf gsrc, gdst, zsrc, zdst;
    const dsdtm_undistort_map* map = nullptr;
    std::vector<int32_t> xy;
    bool init(const dsdtm_undistort_map* m, const dsdtm_camera& cam, const float* dist, Mem src, Mem dst, bool with_depth, int salt) {
        map = m; w = cam.width; h = cam.height; depth = with_depth;
        gs = w + 3; gd = w + 5; zs = w + 1; zd = w + 7;
        xy.resize((size_t)w * h * 2);
        DSDTM::undistort_map_host(cam, dist, xy.data());
        CHECK(gsrc.make(src, extent(gs)) && gdst.make(dst, extent(gd)));
        for (size_t i = 0; i < gsrc.bytes; ++i) ((uint8_t*)gsrc.p)[i] = (uint8_t)((i * 37 + (size_t)salt * 11) % 251);
        if (depth) {
            CHECK(zsrc.make(src, extent(zs) * 2) && zdst.make(dst, extent(zd) * 2));
            for (size_t i = 0; i < zsrc.bytes / 2; ++i) ((uint16_t*)zsrc.p)[i] = (uint16_t)((i * 131 + (size_t)salt) % 5000);
        }
        prefill();
        return true;
    }
    size_t extent(int stride) const { return (size_t)(h - 1) * stride + w; }
    void prefill() { fill_a5(gdst.p, gdst.bytes); if (depth) fill_a5(zdst.p, zdst.bytes); }
    bool untouched() const { return all_a5(gdst.p, gdst.bytes) && (!depth || all_a5(zdst.p, zdst.bytes)); }
    dsdtm_undistort_desc desc() const {
        dsdtm_undistort_desc d{};
        d.map = map; d.gray_src = (const uint8_t*)gsrc.p; d.gray_dst = (uint8_t*)gdst.p; d.gray_src_stride = gs; d.gray_dst_stride = gd;
        if (depth) { d.depth_src = (const uint16_t*)zsrc.p; d.depth_dst = (uint16_t*)zdst.p; d.depth_src_stride = zs; d.depth_dst_stride = zd; }
        return d;
    }
    // every byte of the destinations: the rows by the host function, the padding still 0xA5
    bool answered() const {
        std::vector<uint8_t> g(gdst.bytes, 0xA5);
        std::vector<uint16_t> z(depth ? zdst.bytes / 2 : 0, 0xA5A5);
        DSDTM::undistort_frame_host(xy.data(), w, h, (const uint8_t*)gsrc.p, gs, g.data(), gd, depth ? (const uint16_t*)zsrc.p : nullptr, zs,
                                    depth ? z.data() : nullptr, zd);
        CHECK(memcmp(g.data(), gdst.p, gdst.bytes) == 0);
        CHECK(!depth || memcmp(z.data(), zdst.p, zdst.bytes) == 0);
        return true;
    }
};

struct World {
    dsdtm_undistort_ctx* ctx = nullptr;
    dsdtm_camera cam_a = camera(21, 9), cam_b = camera(8, 12);
    dsdtm_undistort_map* map_a = nullptr;
    dsdtm_undistort_map* map_b = nullptr;
    Frame f[5];
    std::vector<dsdtm_undistort_desc> d;
    bool init() {
        CHECK(dsdtm_undistort_create(0, &ctx) == DSDTM_OK);
        CHECK(dsdtm_undistort_map_create(ctx, &cam_a, DIST_A, &map_a) == DSDTM_OK && dsdtm_undistort_map_create(ctx, &cam_b, DIST_B, &map_b) == DSDTM_OK);
        // pageable -> host, pinned -> device, device -> device, gray only pageable -> pinned host, the second map device -> pageable
        CHECK(f[0].init(map_a, cam_a, DIST_A, PAGEABLE, PAGEABLE, true, 1) && f[1].init(map_a, cam_a, DIST_A, PINNED, DEVICE, true, 2) &&
              f[2].init(map_a, cam_a, DIST_A, DEVICE, DEVICE, true, 3) && f[3].init(map_a, cam_a, DIST_A, PAGEABLE, PINNED, false, 4) &&
              f[4].init(map_b, cam_b, DIST_B, DEVICE, PAGEABLE, true, 5));
        sync();
        return true;
    }
    void sync() { d.clear(); for (auto& x : f) d.push_back(x.desc()); }
    void prefill() { for (auto& x : f) x.prefill(); }
    bool untouched() const { for (auto& x : f) if (!x.untouched()) return false; return true; }
    bool host_untouched() const { for (auto& x : f) if (x.gdst.mem != DEVICE && !x.untouched()) return false; return true; }
    bool answered() const { for (auto& x : f) CHECK(x.answered()); return true; }
    int run() { return dsdtm_undistort_frames(ctx, (int)d.size(), d.data()); }
    ~World() {
        for (auto& x : f) { x.gsrc.release(); x.gdst.release(); x.zsrc.release(); x.zdst.release(); }
        dsdtm_undistort_map_destroy(map_a); dsdtm_undistort_map_destroy(map_b);
        dsdtm_undistort_destroy(ctx);
    }
};

// the map against the host function; five frames of every memory kind and two maps in ONE upload, ONE launch, one read-back, one wait;
// each frame equal to its single call; the points entry
static bool answers_and_memory_kinds() {
    {
        World s;
        CHECK(s.init());
        std::vector<int32_t> got(s.f[0].xy.size(), 0x5A5A5A5A);
        CHECK(dsdtm_undistort_map_read(s.ctx, s.map_a, got.data()) == DSDTM_OK && got == s.f[0].xy);
        got.assign(s.f[4].xy.size(), 0);
        CHECK(dsdtm_undistort_map_read(s.ctx, s.map_b, got.data()) == DSDTM_OK && got == s.f[4].xy);
        const long l0 = fake_undistort_launches(), c0 = fake_hip_calls("hipMemcpyAsync"), s0 = fake_hip_calls("hipStreamSynchronize");
        CHECK(dsdtm_undistort_frames(s.ctx, 0, nullptr) == DSDTM_OK && fake_undistort_launches() == l0 && fake_hip_calls("hipMemcpyAsync") == c0);
        CHECK(s.run() == DSDTM_OK && s.answered());
        CHECK(fake_undistort_launches() == l0 + 1 && fake_hip_calls("hipMemcpyAsync") == c0 + 2 && fake_hip_pending() == 0);
        CHECK(fake_hip_calls("hipStreamSynchronize") == s0 + 2);          // the fake launch's drain and the call's one wait
        for (size_t k = 0; k < s.d.size(); ++k) {                         // singles
            s.prefill();
            CHECK(dsdtm_undistort_frames(s.ctx, 1, &s.d[k]) == DSDTM_OK && s.f[k].answered());
            for (size_t j = 0; j < s.d.size(); ++j) CHECK(j == k || s.f[j].untouched());
        }
        // device destinations only: nothing is read back
        const long c1 = fake_hip_calls("hipMemcpyAsync");
        s.prefill();
        CHECK(dsdtm_undistort_frames(s.ctx, 2, &s.d[1]) == DSDTM_OK && s.f[1].answered() && s.f[2].answered() && fake_hip_calls("hipMemcpyAsync") == c1 + 1);
        // the full batch: one source, 1024 destinations in one device block
        {
            Buf all;
            const size_t each = 21 * 9;
            CHECK(all.make(DEVICE, each * DSDTM_UNDISTORT_MAX_FRAMES));
            std::vector<dsdtm_undistort_desc> full((size_t)DSDTM_UNDISTORT_MAX_FRAMES, s.d[2]);
            for (size_t k = 0; k < full.size(); ++k) { full[k].gray_dst = (uint8_t*)all.p + k * each; full[k].gray_dst_stride = 21; full[k].depth_src = nullptr; full[k].depth_dst = nullptr; }
            CHECK(dsdtm_undistort_frames(s.ctx, (int)full.size(), full.data()) == DSDTM_OK);
            CHECK(memcmp(all.p, (uint8_t*)all.p + each * (DSDTM_UNDISTORT_MAX_FRAMES - 1), each) == 0);
        }
        // points: every other pixel skipped; in place
        const int n = 300;
        std::vector<float> px(2 * n), want_px(2 * n);
        std::vector<uint8_t> skip(n);
        std::vector<double> b(3 * n, 7.0), want_b(3 * n, 7.0);
        for (int i = 0; i < n; ++i) { px[2 * i] = (float)(i % 21) + 0.25f; px[2 * i + 1] = (float)(i % 9) - 0.5f; skip[i] = (uint8_t)(i % 2); }
        DSDTM::undistort_points_host(s.cam_a, DIST_A, n, px.data(), skip.data(), want_px.data(), want_b.data());
        const long l1 = fake_undistort_launches(), c2 = fake_hip_calls("hipMemcpyAsync");
        CHECK(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, n, px.data(), skip.data(), px.data(), b.data()) == DSDTM_OK);
        CHECK(px == want_px && memcmp(b.data(), want_b.data(), b.size() * 8) == 0 && b[3] == 7.0 && b[0] != 7.0);
        CHECK(fake_undistort_launches() == l1 + 1 && fake_hip_calls("hipMemcpyAsync") == c2 + 2 && fake_hip_pending() == 0);
        std::vector<float> out(2 * n, -1.0f);
        DSDTM::undistort_points_host(s.cam_a, DIST_A, n, want_px.data(), nullptr, want_px.data(), want_b.data());
        CHECK(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, n, px.data(), nullptr, out.data(), b.data()) == DSDTM_OK && out == want_px &&
              memcmp(b.data(), want_b.data(), b.size() * 8) == 0);
        CHECK(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, 0, nullptr, nullptr, nullptr, nullptr) == DSDTM_OK && fake_undistort_launches() == l1 + 2);
        std::vector<float> big(2 * (size_t)DSDTM_UNDISTORT_MAX_POINTS, 3.0f);
        std::vector<double> big_b(3 * (size_t)DSDTM_UNDISTORT_MAX_POINTS);
        CHECK(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, DSDTM_UNDISTORT_MAX_POINTS, big.data(), nullptr, big.data(), big_b.data()) == DSDTM_OK);
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

static bool invalid(World& s, int rc, const char* a, const char* b, long l0, long c0) {
    const char* e = dsdtm_undistort_last_error(s.ctx);
    if (rc != DSDTM_ERR_INVALID || !s.untouched() || !strstr(e, a) || !strstr(e, b) || fake_undistort_launches() != l0 || fake_hip_calls("hipMemcpyAsync") != c0 ||
        fake_hip_pending() != 0) {
        std::fprintf(stderr, "expected INVALID naming '%s' and '%s': rc %d, error '%s'\n", a, b, rc, e);
        return false;
    }
    return true;
}

// every refusal of U1, U4 and U5: named, nothing enqueued, every output untouched
static bool refusals() {
    {
        World s;
        CHECK(s.init());
        const long l0 = fake_undistort_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        // U1
        dsdtm_undistort_map* const stale = (dsdtm_undistort_map*)(uintptr_t)1;
        dsdtm_undistort_map* m = stale;
        auto map_refused = [&](dsdtm_camera cam, const float* dist, const char* what) {
            m = stale;
            const int rc = dsdtm_undistort_map_create(s.ctx, &cam, dist, &m);
            return m == nullptr && invalid(s, rc, "undistort_map_create", what, l0, c0);
        };
        dsdtm_camera c = s.cam_a;
        c.width = 7; CHECK(map_refused(c, DIST_A, "width")); c.width = 4097; CHECK(map_refused(c, DIST_A, "width")); c = s.cam_a;
        c.height = 7; CHECK(map_refused(c, DIST_A, "height")); c.height = 4097; CHECK(map_refused(c, DIST_A, "height")); c = s.cam_a;
        c.fx = 0.0f; CHECK(map_refused(c, DIST_A, "fx")); c.fx = -1.0f; CHECK(map_refused(c, DIST_A, "fx")); c.fx = nan; CHECK(map_refused(c, DIST_A, "fx")); c = s.cam_a;
        c.fy = 0.0f; CHECK(map_refused(c, DIST_A, "fy")); c.fy = inf; CHECK(map_refused(c, DIST_A, "fy")); c = s.cam_a;
        c.cx = nan; CHECK(map_refused(c, DIST_A, "cx")); c = s.cam_a;
        c.cy = -inf; CHECK(map_refused(c, DIST_A, "cy")); c = s.cam_a;
        static const char* const coef[5] = {"k1", "k2", "p1", "p2", "k3"};
        for (int i = 0; i < 5; ++i) {
            float dist[5];
            memcpy(dist, DIST_A, sizeof dist);
            dist[i] = i % 2 ? nan : inf;
            CHECK(map_refused(c, dist, coef[i]));
        }
        CHECK(dsdtm_undistort_map_create(s.ctx, nullptr, DIST_A, &m) == DSDTM_ERR_INVALID && strstr(dsdtm_undistort_last_error(s.ctx), "cam is NULL"));
        CHECK(dsdtm_undistort_map_create(s.ctx, &c, nullptr, &m) == DSDTM_ERR_INVALID && strstr(dsdtm_undistort_last_error(s.ctx), "dist is NULL"));
        CHECK(dsdtm_undistort_map_create(s.ctx, &c, DIST_A, nullptr) == DSDTM_ERR_INVALID && dsdtm_undistort_map_create(nullptr, &c, DIST_A, &m) == DSDTM_ERR_INVALID);
        c.width = 8; c.height = 8;          // the smallest map is accepted
        CHECK(dsdtm_undistort_map_create(s.ctx, &c, DIST_A, &m) == DSDTM_OK && m);
        dsdtm_undistort_map_destroy(m);
        dsdtm_undistort_map_destroy(nullptr);
        int32_t word = 0x5A5A5A5A;
        CHECK(dsdtm_undistort_map_read(s.ctx, nullptr, &word) == DSDTM_ERR_INVALID && dsdtm_undistort_map_read(s.ctx, s.map_a, nullptr) == DSDTM_ERR_INVALID &&
              dsdtm_undistort_map_read(nullptr, s.map_a, &word) == DSDTM_ERR_INVALID && word == 0x5A5A5A5A);
        // U4
        const long l1 = fake_undistort_launches(), c1 = fake_hip_calls("hipMemcpyAsync");
        CHECK(dsdtm_undistort_frames(nullptr, 0, nullptr) == DSDTM_ERR_INVALID);
        CHECK(invalid(s, dsdtm_undistort_frames(s.ctx, -1, s.d.data()), "n = -1", "0..1024", l1, c1));
        CHECK(invalid(s, dsdtm_undistort_frames(s.ctx, 1025, s.d.data()), "n = 1025", "0..1024", l1, c1));
        CHECK(invalid(s, dsdtm_undistort_frames(s.ctx, 3, nullptr), "undistort_frames", "descs is NULL", l1, c1));
        auto& d = s.d[3];
        const dsdtm_undistort_desc good3 = d;
        d.map = nullptr; CHECK(invalid(s, s.run(), "frame 3", "map is NULL", l1, c1)); d = good3;
        d.gray_src = nullptr; CHECK(invalid(s, s.run(), "frame 3", "gray_src is NULL", l1, c1)); d = good3;
        d.gray_dst = nullptr; CHECK(invalid(s, s.run(), "frame 3", "gray_dst is NULL", l1, c1)); d = good3;
        d.gray_src_stride = 20; CHECK(invalid(s, s.run(), "frame 3", "gray_src_stride below width", l1, c1)); d = good3;
        d.gray_dst_stride = 20; CHECK(invalid(s, s.run(), "frame 3", "gray_dst_stride below width", l1, c1)); d = good3;
        d.depth_src = (const uint16_t*)s.f[0].zsrc.p; d.depth_src_stride = 22; CHECK(invalid(s, s.run(), "frame 3", "depth_dst is NULL", l1, c1)); d = good3;
        auto& d2 = s.d[2];
        const dsdtm_undistort_desc good2 = d2;
        d2.depth_src = nullptr; CHECK(invalid(s, s.run(), "frame 2", "depth_src is NULL", l1, c1)); d2 = good2;
        d2.depth_src_stride = 20; CHECK(invalid(s, s.run(), "frame 2", "depth_src_stride below width", l1, c1)); d2 = good2;
        d2.depth_dst_stride = 0; CHECK(invalid(s, s.run(), "frame 2", "depth_dst_stride below width", l1, c1)); d2 = good2;
        // a destination that meets a source (its own, another frame's) or another destination; sources may be shared
        d2.gray_dst = (uint8_t*)d2.gray_src + 5; CHECK(invalid(s, s.run(), "frame 2: gray_dst overlaps", "gray_src of frame 2", l1, c1)); d2 = good2;
        d2.depth_dst = (uint16_t*)s.d[4].depth_src; CHECK(invalid(s, s.run(), "frame 2: depth_dst overlaps", "depth_src of frame 4", l1, c1)); d2 = good2;
        d2.gray_dst = s.d[1].gray_dst + (s.f[1].extent(s.f[1].gd) - 1);      // the last byte of frame 1's extent
        CHECK(invalid(s, s.run(), "gray_dst overlaps", "gray_dst of frame", l1, c1)); d2 = good2;
        d2.gray_src = s.d[1].gray_src;          // (the pinned source, twice: legal)
        d2.depth_src = s.d[1].depth_src;
        CHECK(s.run() == DSDTM_OK);
        d2 = good2;
        s.prefill();
        // another device: a context on device 1 (the fake's device memory is device 0's)
        dsdtm_undistort_ctx* other = nullptr;
        dsdtm_undistort_map* other_map = nullptr;
        CHECK(dsdtm_undistort_create(1, &other) == DSDTM_OK && dsdtm_undistort_map_create(other, &s.cam_a, DIST_A, &other_map) == DSDTM_OK);
        const long l2 = fake_undistort_launches(), c2 = fake_hip_calls("hipMemcpyAsync");
        CHECK(dsdtm_undistort_frames(other, 1, &s.d[0]) == DSDTM_ERR_INVALID && strstr(dsdtm_undistort_last_error(other), "frame 0: map lies on another device"));
        CHECK(dsdtm_undistort_map_read(other, s.map_a, &word) == DSDTM_ERR_INVALID && word == 0x5A5A5A5A);
        dsdtm_undistort_desc od = s.d[2];
        od.map = other_map;
        CHECK(dsdtm_undistort_frames(other, 1, &od) == DSDTM_ERR_INVALID && strstr(dsdtm_undistort_last_error(other), "frame 0: gray_src lies in another device's memory"));
        od.gray_src = s.d[0].gray_src; od.depth_src = s.d[0].depth_src; od.gray_src_stride = s.d[0].gray_src_stride; od.depth_src_stride = s.d[0].depth_src_stride;
        CHECK(dsdtm_undistort_frames(other, 1, &od) == DSDTM_ERR_INVALID && strstr(dsdtm_undistort_last_error(other), "frame 0: gray_dst lies in another device's memory"));
        CHECK(s.untouched() && fake_undistort_launches() == l2 && fake_hip_calls("hipMemcpyAsync") == c2);
        dsdtm_undistort_map_destroy(other_map);
        dsdtm_undistort_destroy(other);
        // U5
        const int n = 40;
        std::vector<float> px(2 * n, 4.0f), out(2 * n);
        std::vector<double> b(3 * n);
        fill_a5(out.data(), out.size() * 4); fill_a5(b.data(), b.size() * 8);
        auto points_refused = [&](int rc, const char* what) {
            return all_a5(out.data(), out.size() * 4) && all_a5(b.data(), b.size() * 8) && invalid(s, rc, "undistort_points", what, l2, c2);
        };
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, -1, px.data(), nullptr, out.data(), b.data()), "n = -1"));
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, 16385, px.data(), nullptr, out.data(), b.data()), "n = 16385"));
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, n, nullptr, nullptr, out.data(), b.data()), "px_in is NULL"));
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, n, px.data(), nullptr, nullptr, b.data()), "px_out is NULL"));
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, n, px.data(), nullptr, out.data(), nullptr), "bearing_out is NULL"));
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, nullptr, DIST_A, n, px.data(), nullptr, out.data(), b.data()), "cam is NULL"));
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, &s.cam_a, nullptr, n, px.data(), nullptr, out.data(), b.data()), "dist is NULL"));
        px[2 * 17 + 1] = nan;
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, n, px.data(), nullptr, out.data(), b.data()), "px_in is not finite at index 17"));
        px[2 * 17 + 1] = 4.0f; px[2 * 39] = inf;
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, n, px.data(), nullptr, out.data(), b.data()), "px_in is not finite at index 39"));
        px[2 * 39] = 4.0f;
        c = s.cam_a; c.fy = 0.0f;
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, &c, DIST_A, n, px.data(), nullptr, out.data(), b.data()), "fy"));
        float dist[5] = {0, 0, nan, 0, 0};
        CHECK(points_refused(dsdtm_undistort_points(s.ctx, &s.cam_a, dist, n, px.data(), nullptr, out.data(), b.data()), "p1"));
        c = s.cam_a; c.width = 0; c.height = -3;          // not read by the points entry
        CHECK(dsdtm_undistort_points(s.ctx, &c, DIST_A, n, px.data(), nullptr, out.data(), b.data()) == DSDTM_OK);
        CHECK(dsdtm_undistort_points(nullptr, &s.cam_a, DIST_A, n, px.data(), nullptr, out.data(), b.data()) == DSDTM_ERR_INVALID);
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

// every HIP call of every entry failing once: an error with a text, every host output untouched, nothing pending (what was enqueued in
// front of the failure has been waited for: the pinned block is the next call's), nothing leaked; the next call succeeds
static bool call_failures() {
    {
        World s;
        CHECK(s.init());
        CHECK(s.run() == DSDTM_OK);          // (the staging block has its size)
        const size_t live0 = fake_hip_live_allocations();
        struct Inject { const char* api; long nth; };
        auto frames_fail = [&](Inject in) {
            s.prefill();
            if (in.api) fake_hip_fail(in.api, in.nth); else fake_undistort_fail(1);
            const int rc = s.run();
            if (in.api) fake_hip_fail(in.api, 0); else fake_undistort_fail(0);
            CHECK(rc == DSDTM_ERR_HIP && fake_hip_pending() == 0 && strlen(dsdtm_undistort_last_error(s.ctx)) > 0 && s.host_untouched());
            s.prefill();
            CHECK(s.run() == DSDTM_OK && s.answered() && fake_hip_live_allocations() == live0);
            return true;
        };
        // the device, the pinned source's device view, the upload, the launch, the read-back (upload and launch pending in front of it),
        // the fake launch's drain, the wait
        for (Inject in : {Inject{"hipSetDevice", 1}, Inject{"hipHostGetDevicePointer", 1}, Inject{"hipHostGetDevicePointer", 2}, Inject{"hipMemcpyAsync", 1},
                          Inject{nullptr, 1}, Inject{"hipMemcpyAsync", 2}, Inject{"hipStreamSynchronize", 1}, Inject{"hipStreamSynchronize", 2}})
            CHECK(frames_fail(in));
        // a staging block that must grow cannot be had: a fresh context, pinned then device; then it grows and the call succeeds
        for (const char* api : {"hipHostMalloc", "hipMalloc"}) {
            dsdtm_undistort_ctx* keep = s.ctx;
            CHECK(dsdtm_undistort_create(0, &s.ctx) == DSDTM_OK);
            s.prefill();
            fake_hip_fail(api, 1);
            const int rc = s.run();
            fake_hip_fail(api, 0);
            CHECK(rc == DSDTM_ERR_HIP && s.untouched() && fake_hip_pending() == 0);
            CHECK(s.run() == DSDTM_OK && s.answered());
            dsdtm_undistort_destroy(s.ctx);
            s.ctx = keep;
        }
        // the map: its allocation, its launch, its wait — no map comes out, nothing leaks
        for (Inject in : {Inject{"hipSetDevice", 1}, Inject{"hipMalloc", 1}, Inject{nullptr, 1}, Inject{"hipStreamSynchronize", 1}, Inject{"hipStreamSynchronize", 2}}) {
            dsdtm_undistort_map* m = (dsdtm_undistort_map*)(uintptr_t)1;
            if (in.api) fake_hip_fail(in.api, in.nth); else fake_undistort_fail(1);
            const int rc = dsdtm_undistort_map_create(s.ctx, &s.cam_b, DIST_B, &m);
            if (in.api) fake_hip_fail(in.api, 0); else fake_undistort_fail(0);
            CHECK(rc == DSDTM_ERR_HIP && m == nullptr && fake_hip_pending() == 0 && fake_hip_live_allocations() == live0 && strlen(dsdtm_undistort_last_error(s.ctx)) > 0);
        }
        // map_read: the copy, the wait
        std::vector<int32_t> got(s.f[0].xy.size());
        for (Inject in : {Inject{"hipSetDevice", 1}, Inject{"hipMemcpyAsync", 1}, Inject{"hipStreamSynchronize", 1}}) {
            fill_a5(got.data(), got.size() * 4);
            fake_hip_fail(in.api, in.nth);
            const int rc = dsdtm_undistort_map_read(s.ctx, s.map_a, got.data());
            fake_hip_fail(in.api, 0);
            CHECK(rc == DSDTM_ERR_HIP && all_a5(got.data(), got.size() * 4) && fake_hip_pending() == 0);
        }
        CHECK(dsdtm_undistort_map_read(s.ctx, s.map_a, got.data()) == DSDTM_OK && got == s.f[0].xy);
        // points
        const int n = 70;
        std::vector<float> px(2 * n, 5.5f), out(2 * n), want(2 * n);
        std::vector<double> b(3 * n), want_b(3 * n);
        DSDTM::undistort_points_host(s.cam_a, DIST_A, n, px.data(), nullptr, want.data(), want_b.data());
        for (Inject in : {Inject{"hipMemcpyAsync", 1}, Inject{nullptr, 1}, Inject{"hipMemcpyAsync", 2}, Inject{"hipStreamSynchronize", 1}, Inject{"hipStreamSynchronize", 2}}) {
            fill_a5(out.data(), out.size() * 4); fill_a5(b.data(), b.size() * 8);
            if (in.api) fake_hip_fail(in.api, in.nth); else fake_undistort_fail(1);
            const int rc = dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, n, px.data(), nullptr, out.data(), b.data());
            if (in.api) fake_hip_fail(in.api, 0); else fake_undistort_fail(0);
            CHECK(rc == DSDTM_ERR_HIP && all_a5(out.data(), out.size() * 4) && all_a5(b.data(), b.size() * 8) && fake_hip_pending() == 0);
            CHECK(dsdtm_undistort_points(s.ctx, &s.cam_a, DIST_A, n, px.data(), nullptr, out.data(), b.data()) == DSDTM_OK && out == want &&
                  memcmp(b.data(), want_b.data(), b.size() * 8) == 0);
        }
        CHECK(fake_hip_live_allocations() == live0);
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_undistort", dsdtm_undistort_create, dsdtm_undistort_destroy, dsdtm_undistort_last_error);
}

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
