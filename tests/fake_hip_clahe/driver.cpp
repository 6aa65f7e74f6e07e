// libdsdtm_amd_clahe.so's host side (dsdtm_amd/csrc/clahe_api.cpp) against the fake HIP runtime of tests/fake_hip (unmodified): the
// context, the checks, the three memory kinds of a source and the two of a destination, the tables asked for and not, the one upload /
// two launches / one read-back / one wait, the growth of the staging blocks, every refusal and every HIP call failing in turn — as a
// stand-alone program under ASan/UBSan/LSan. The launches are the fakes of tests/fake_hip_clahe/fake_clahe.cpp. (The fake runtime never
// reports a stream capture, so that refusal is not reached here.) Test infrastructure (tests/test_clahe_cpu.py); nothing here is part
// of the product.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_clahe.h"
#include "../../dsdtm_amd/host/dsdtm_clahe_host.hpp"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_clahe.h"

enum Mem { PAGEABLE, PINNED, DEVICE };

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

// one frame: the source filled from a pattern, the destination and the tables prefilled with 0xA5; strides wider than the width
struct Frame {
    int w = 0, h = 0, ss = 0, ds = 0, tx = 0, ty = 0;
    double clip = 3.0;
    bool want_luts = false;
    Buf src, dst;
    std::vector<uint8_t> luts;
    bool init(int w_, int h_, Mem smem, Mem dmem, double clip_, int tx_, int ty_, bool want_luts_, int salt) {
        w = w_; h = h_; clip = clip_; tx = tx_; ty = ty_; want_luts = want_luts_;
        ss = w + 3; ds = w + 5;
        CHECK(src.make(smem, extent(ss)) && dst.make(dmem, extent(ds)));
        for (size_t i = 0; i < src.bytes; ++i) ((uint8_t*)src.p)[i] = (uint8_t)(((i * 37 + (size_t)salt * 11) % 251) / (1 + i % 3));
        luts.assign(want_luts ? lut_bytes() + 7 : 0, 0xA5);
        prefill();
        return true;
    }
    size_t extent(int stride) const { return (size_t)(h - 1) * stride + w; }
    size_t lut_bytes() const { return (size_t)(tx ? tx : 8) * (size_t)(ty ? ty : 8) * 256; }
    void prefill() { fill_a5(dst.p, dst.bytes); fill_a5(luts.data(), luts.size()); }
    bool untouched() const { return all_a5(dst.p, dst.bytes) && all_a5(luts.data(), luts.size()); }
    dsdtm_clahe_desc desc() {
        dsdtm_clahe_desc d{};
        d.src = (const uint8_t*)src.p; d.dst = (uint8_t*)dst.p; d.lut_out = want_luts ? luts.data() : nullptr; d.clip_limit = clip;
        d.width = w; d.height = h; d.src_stride = ss; d.dst_stride = ds; d.tiles_x = tx; d.tiles_y = ty;
        return d;
    }
    // every byte of the destination and of the tables: the rows by the host function, the padding still 0xA5
    bool answered(bool dst_too = true) const {
        std::vector<uint8_t> want(dst.bytes, 0xA5), want_luts_v(lut_bytes());
        DSDTM::clahe_host((const uint8_t*)src.p, ss, want.data(), ds, w, h, clip, tx, ty, want_luts_v.data());
        if (dst_too) CHECK(memcmp(want.data(), dst.p, dst.bytes) == 0);
        if (want_luts) CHECK(memcmp(want_luts_v.data(), luts.data(), lut_bytes()) == 0 && all_a5(luts.data() + lut_bytes(), 7));
        return true;
    }
};

struct World {
    dsdtm_clahe_ctx* ctx = nullptr;
    Frame f[6];
    std::vector<dsdtm_clahe_desc> d;
    bool init() {
        CHECK(dsdtm_clahe_create(0, &ctx) == DSDTM_OK);
        // pageable -> host with tables, pinned -> device, device -> device with tables (the quirk of E1), pageable -> pinned host
        // (one tile), device -> pageable (16 x 16 tiles, the mirror repeats), pinned -> device without a clip
        CHECK(f[0].init(40, 24, PAGEABLE, PAGEABLE, 3.0, 0, 0, true, 1) && f[1].init(33, 21, PINNED, DEVICE, 3.0, 4, 3, false, 2) &&
              f[2].init(64, 50, DEVICE, DEVICE, 2.0, 8, 8, true, 3) && f[3].init(19, 16, PAGEABLE, PINNED, 40.0, 1, 1, false, 4) &&
              f[4].init(17, 16, DEVICE, PAGEABLE, 3.0, 16, 16, true, 5) && f[5].init(48, 32, PINNED, DEVICE, 0.0, 8, 8, false, 6));
        sync();
        return true;
    }
    void sync() { d.clear(); for (auto& x : f) d.push_back(x.desc()); }
    void prefill() { for (auto& x : f) x.prefill(); }
    bool untouched() const { for (auto& x : f) if (!x.untouched()) return false; return true; }
    bool host_untouched() const { for (auto& x : f) if (!all_a5(x.luts.data(), x.luts.size()) || (x.dst.mem != DEVICE && !all_a5(x.dst.p, x.dst.bytes))) return false; return true; }
    bool answered() const { for (auto& x : f) CHECK(x.answered()); return true; }
    int run() { return dsdtm_clahe_apply_batch(ctx, (int)d.size(), d.data()); }
    ~World() {
        for (auto& x : f) { x.src.release(); x.dst.release(); }
        dsdtm_clahe_destroy(ctx);
    }
};

// six frames of every memory kind and of mixed sizes and grids in ONE upload, TWO launches, one read-back, one wait; each frame equal to
// its single call; the tables entry; n = 0; the staging blocks grow
static bool answers_and_memory_kinds() {
    {
        World s;
        CHECK(s.init());
        const long l0 = fake_clahe_launches(), c0 = fake_hip_calls("hipMemcpyAsync"), s0 = fake_hip_calls("hipStreamSynchronize");
        CHECK(dsdtm_clahe_apply_batch(s.ctx, 0, nullptr) == DSDTM_OK && fake_clahe_launches() == l0 && fake_hip_calls("hipMemcpyAsync") == c0);
        CHECK(s.run() == DSDTM_OK && s.answered());
        CHECK(fake_clahe_launches() == l0 + 2 && fake_hip_calls("hipMemcpyAsync") == c0 + 2 && fake_hip_pending() == 0);
        CHECK(fake_hip_calls("hipStreamSynchronize") == s0 + 3);          // the two fake launches' drains and the call's one wait
        for (size_t k = 0; k < s.d.size(); ++k) {                         // singles
            s.prefill();
            CHECK(dsdtm_clahe_apply(s.ctx, &s.d[k]) == DSDTM_OK && s.f[k].answered());
            for (size_t j = 0; j < s.d.size(); ++j) CHECK(j == k || s.f[j].untouched());
        }
        // device destinations and no tables asked for: nothing is read back
        const long c1 = fake_hip_calls("hipMemcpyAsync");
        s.prefill();
        dsdtm_clahe_desc two[2] = {s.d[1], s.d[5]};
        CHECK(dsdtm_clahe_apply_batch(s.ctx, 2, two) == DSDTM_OK && s.f[1].answered() && s.f[5].answered() && fake_hip_calls("hipMemcpyAsync") == c1 + 1);
        // the tables entry: one launch, the destination is not read (here: NULL) and not written
        const long l1 = fake_clahe_launches();
        s.prefill();
        for (size_t k : {0u, 2u, 4u}) {
            dsdtm_clahe_desc only = s.d[k];
            only.dst = nullptr; only.dst_stride = 0;
            CHECK(dsdtm_clahe_luts(s.ctx, &only) == DSDTM_OK && s.f[k].answered(false) && all_a5(s.f[k].dst.p, s.f[k].dst.bytes));
        }
        CHECK(fake_clahe_launches() == l1 + 3);
        // the staging blocks grow: a fresh context sees a small call, then a larger one (both blocks are re-allocated), then the small one again
        dsdtm_clahe_ctx* fresh = nullptr;
        CHECK(dsdtm_clahe_create(0, &fresh) == DSDTM_OK);
        const long hm0 = fake_hip_calls("hipHostMalloc"), dm0 = fake_hip_calls("hipMalloc");
        s.prefill();
        CHECK(dsdtm_clahe_apply(fresh, &s.d[3]) == DSDTM_OK && s.f[3].answered() && fake_hip_calls("hipHostMalloc") == hm0 + 1 && fake_hip_calls("hipMalloc") == dm0 + 1);
        {
            Frame big;
            CHECK(big.init(700, 300, PAGEABLE, PAGEABLE, 3.0, 16, 16, true, 9));
            dsdtm_clahe_desc bd = big.desc();
            CHECK(dsdtm_clahe_apply(fresh, &bd) == DSDTM_OK && big.answered() && fake_hip_calls("hipHostMalloc") == hm0 + 2 && fake_hip_calls("hipMalloc") == dm0 + 2);
        }
        s.prefill();
        CHECK(dsdtm_clahe_apply(fresh, &s.d[3]) == DSDTM_OK && s.f[3].answered() && fake_hip_calls("hipHostMalloc") == hm0 + 2 && fake_hip_calls("hipMalloc") == dm0 + 2);
        dsdtm_clahe_destroy(fresh);
        // the full batch: one device source, 1024 destinations in one device block
        {
            Buf all;
            const size_t each = 33 * 21;
            CHECK(all.make(DEVICE, each * DSDTM_CLAHE_MAX_FRAMES));
            std::vector<dsdtm_clahe_desc> full((size_t)DSDTM_CLAHE_MAX_FRAMES, s.d[2]);
            for (size_t k = 0; k < full.size(); ++k) {
                full[k] = s.d[1]; full[k].src = (const uint8_t*)s.f[2].src.p; full[k].src_stride = 67;          // (frame 2's device buffer, read as 33 x 21)
                full[k].dst = (uint8_t*)all.p + k * each; full[k].dst_stride = 33;
            }
            CHECK(dsdtm_clahe_apply_batch(s.ctx, (int)full.size(), full.data()) == DSDTM_OK);
            CHECK(memcmp(all.p, (uint8_t*)all.p + each * (DSDTM_CLAHE_MAX_FRAMES - 1), each) == 0);
        }
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

static bool invalid(World& s, int rc, const char* a, const char* b, long l0, long c0) {
    const char* e = dsdtm_clahe_last_error(s.ctx);
    if (rc != DSDTM_ERR_INVALID || !s.untouched() || !strstr(e, a) || !strstr(e, b) || fake_clahe_launches() != l0 || fake_hip_calls("hipMemcpyAsync") != c0 ||
        fake_hip_pending() != 0) {
        std::fprintf(stderr, "expected INVALID naming '%s' and '%s': rc %d, error '%s'\n", a, b, rc, e);
        return false;
    }
    std::printf("ok refusal: %s\n", b);
    return true;
}

// every refusal: named with its desc, nothing enqueued, every output of EVERY frame untouched (all or nothing)
static bool refusals() {
    {
        World s;
        CHECK(s.init());
        const long l0 = fake_clahe_launches(), c0 = fake_hip_calls("hipMemcpyAsync");
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        CHECK(dsdtm_clahe_apply_batch(nullptr, 0, nullptr) == DSDTM_ERR_INVALID && dsdtm_clahe_apply(nullptr, &s.d[0]) == DSDTM_ERR_INVALID &&
              dsdtm_clahe_luts(nullptr, &s.d[0]) == DSDTM_ERR_INVALID);
        CHECK(invalid(s, dsdtm_clahe_apply_batch(s.ctx, -1, s.d.data()), "n = -1", "0..1024", l0, c0));
        CHECK(invalid(s, dsdtm_clahe_apply_batch(s.ctx, 1025, s.d.data()), "n = 1025", "0..1024", l0, c0));
        CHECK(invalid(s, dsdtm_clahe_apply_batch(s.ctx, 3, nullptr), "clahe_apply_batch", "descs is NULL", l0, c0));
        CHECK(invalid(s, dsdtm_clahe_apply(s.ctx, nullptr), "clahe_apply", "desc is NULL", l0, c0));
        CHECK(invalid(s, dsdtm_clahe_luts(s.ctx, nullptr), "clahe_luts", "desc is NULL", l0, c0));
        // a field of desc 4 (the frames in front of it are good: all or nothing)
        auto& d = s.d[4];
        const dsdtm_clahe_desc good = d;
        d.width = 15; CHECK(invalid(s, s.run(), "desc 4", "width out of range", l0, c0)); d.width = 4097; CHECK(invalid(s, s.run(), "desc 4", "width out of range", l0, c0)); d = good;
        d.height = 15; CHECK(invalid(s, s.run(), "desc 4", "height out of range", l0, c0)); d.height = 4097; CHECK(invalid(s, s.run(), "desc 4", "height out of range", l0, c0)); d = good;
        d.tiles_x = 17; CHECK(invalid(s, s.run(), "desc 4", "tiles_x out of range", l0, c0)); d.tiles_x = -1; CHECK(invalid(s, s.run(), "desc 4", "tiles_x out of range", l0, c0)); d = good;
        d.tiles_y = 17; CHECK(invalid(s, s.run(), "desc 4", "tiles_y out of range", l0, c0)); d.tiles_y = -2; CHECK(invalid(s, s.run(), "desc 4", "tiles_y out of range", l0, c0)); d = good;
        for (double bad : {nan, inf, -inf, -0.5}) { d.clip_limit = bad; CHECK(invalid(s, s.run(), "desc 4", "clip_limit is not a finite number at or above 0", l0, c0)); }
        d = good;
        d.src = nullptr; CHECK(invalid(s, s.run(), "desc 4", "src is NULL", l0, c0)); d = good;
        d.dst = nullptr; CHECK(invalid(s, s.run(), "desc 4", "dst is NULL", l0, c0)); d = good;
        d.src_stride = 16; CHECK(invalid(s, s.run(), "desc 4", "src_stride below width", l0, c0)); d = good;
        d.dst_stride = 0; CHECK(invalid(s, s.run(), "desc 4", "dst_stride below width", l0, c0)); d = good;
        d.lut_out = nullptr; CHECK(invalid(s, dsdtm_clahe_luts(s.ctx, &d), "clahe_luts: desc 0", "lut_out is NULL", l0, c0)); d = good;
        d.lut_out = (uint8_t*)s.f[2].dst.p; CHECK(invalid(s, s.run(), "desc 4", "lut_out lies in device memory", l0, c0)); d = good;
        // a destination that meets a source (its own, another frame's), another destination or somebody's tables; sources may be shared
        auto& d2 = s.d[2];
        const dsdtm_clahe_desc good2 = d2;
        d2.dst = (uint8_t*)d2.src + 5; CHECK(invalid(s, s.run(), "desc 2: dst overlaps", "src of desc 2", l0, c0)); d2 = good2;
        d2.dst = (uint8_t*)s.d[4].src; d2.width = 17; d2.height = 16; d2.src_stride = 67; d2.dst_stride = 20;
        CHECK(invalid(s, s.run(), "desc 2: dst overlaps", "src of desc 4", l0, c0)); d2 = good2;
        d2.dst = s.d[1].dst + (s.f[1].extent(s.f[1].ds) - 1);      // the last byte of frame 1's extent
        CHECK(invalid(s, s.run(), "dst overlaps", "dst of desc", l0, c0)); d2 = good2;
        s.d[0].lut_out = s.d[0].dst + 3; CHECK(invalid(s, s.run(), "desc 0", "lut_out overlaps dst of desc 0", l0, c0)); s.d[0] = s.f[0].desc();
        s.d[0].lut_out = s.d[4].lut_out; CHECK(invalid(s, s.run(), "lut_out overlaps", "lut_out of desc", l0, c0)); s.d[0] = s.f[0].desc();
        d2.src = s.d[1].src; d2.width = 33; d2.height = 21; d2.src_stride = 36; d2.dst_stride = 69; d2.lut_out = nullptr;          // (the pinned source, twice: legal)
        CHECK(s.run() == DSDTM_OK);
        d2 = good2;
        s.prefill();
        // another device: a context on device 1 (the fake's device memory is device 0's)
        dsdtm_clahe_ctx* other = nullptr;
        CHECK(dsdtm_clahe_create(1, &other) == DSDTM_OK);
        const long l2 = fake_clahe_launches(), c2 = fake_hip_calls("hipMemcpyAsync");
        CHECK(dsdtm_clahe_apply(other, &s.d[2]) == DSDTM_ERR_INVALID && strstr(dsdtm_clahe_last_error(other), "desc 0: src lies in another device's memory"));
        CHECK(dsdtm_clahe_apply(other, &s.d[1]) == DSDTM_ERR_INVALID && strstr(dsdtm_clahe_last_error(other), "desc 0: dst lies in another device's memory"));
        CHECK(s.untouched() && fake_clahe_launches() == l2 && fake_hip_calls("hipMemcpyAsync") == c2);
        CHECK(dsdtm_clahe_apply(other, &s.d[0]) == DSDTM_OK && s.f[0].answered());          // (host memory is anybody's)
        dsdtm_clahe_destroy(other);
        // the smallest and the largest accepted: 16 x 16 with 16 x 16 tiles of one pixel; clip limits at the edges of E2
        Frame tiny;
        CHECK(tiny.init(16, 16, PAGEABLE, PAGEABLE, 1e300, 16, 16, true, 7));
        dsdtm_clahe_desc td = tiny.desc();
        CHECK(dsdtm_clahe_apply(s.ctx, &td) == DSDTM_OK && tiny.answered());
        tiny.clip = 1e-300; tiny.prefill(); td = tiny.desc();
        CHECK(dsdtm_clahe_apply(s.ctx, &td) == DSDTM_OK && tiny.answered());
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

// every HIP call of the entry failing once: an error with a text, every host output untouched, nothing pending (what was enqueued in
// front of the failure has been waited for: the pinned block is the next call's), nothing leaked; the next call succeeds
static bool call_failures() {
    {
        World s;
        CHECK(s.init());
        CHECK(s.run() == DSDTM_OK);          // (the staging block has its size)
        const size_t live0 = fake_hip_live_allocations();
        struct Inject { const char* api; long nth; };
        // the device, the pinned sources' device views, the upload, the two launches, the read-back, the fake launches' drains, the wait
        for (Inject in : {Inject{"hipSetDevice", 1}, Inject{"hipHostGetDevicePointer", 1}, Inject{"hipHostGetDevicePointer", 2}, Inject{"hipMemcpyAsync", 1},
                          Inject{nullptr, 1}, Inject{nullptr, 2}, Inject{"hipMemcpyAsync", 2}, Inject{"hipStreamSynchronize", 1}, Inject{"hipStreamSynchronize", 2},
                          Inject{"hipStreamSynchronize", 3}}) {
            s.prefill();
            if (in.api) fake_hip_fail(in.api, in.nth); else fake_clahe_fail(in.nth);
            const int rc = s.run();
            if (in.api) fake_hip_fail(in.api, 0); else fake_clahe_fail(0);
            CHECK(rc == DSDTM_ERR_HIP && fake_hip_pending() == 0 && strlen(dsdtm_clahe_last_error(s.ctx)) > 0 && s.host_untouched());
            s.prefill();
            CHECK(s.run() == DSDTM_OK && s.answered() && fake_hip_live_allocations() == live0);
        }
        // a staging block that must grow cannot be had: a fresh context, pinned then device; then it grows and the call succeeds
        for (const char* api : {"hipHostMalloc", "hipMalloc"}) {
            dsdtm_clahe_ctx* keep = s.ctx;
            CHECK(dsdtm_clahe_create(0, &s.ctx) == DSDTM_OK);
            s.prefill();
            fake_hip_fail(api, 1);
            const int rc = s.run();
            fake_hip_fail(api, 0);
            CHECK(rc == DSDTM_ERR_HIP && s.untouched() && fake_hip_pending() == 0);
            CHECK(s.run() == DSDTM_OK && s.answered());
            dsdtm_clahe_destroy(s.ctx);
            s.ctx = keep;
        }
        // the tables entry: its launch, its read-back, its wait
        for (Inject in : {Inject{nullptr, 1}, Inject{"hipMemcpyAsync", 2}, Inject{"hipStreamSynchronize", 2}}) {
            s.prefill();
            if (in.api) fake_hip_fail(in.api, in.nth); else fake_clahe_fail(in.nth);
            const int rc = dsdtm_clahe_luts(s.ctx, &s.d[0]);
            if (in.api) fake_hip_fail(in.api, 0); else fake_clahe_fail(0);
            CHECK(rc == DSDTM_ERR_HIP && fake_hip_pending() == 0 && s.untouched());
            CHECK(dsdtm_clahe_luts(s.ctx, &s.d[0]) == DSDTM_OK && s.f[0].answered(false));
        }
        CHECK(fake_hip_live_allocations() == live0);
    }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_clahe", dsdtm_clahe_create, dsdtm_clahe_destroy, dsdtm_clahe_last_error);
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
