// dsdtm_track_frames against the fake HIP runtime of tests/fake_hip (unmodified): the host side of the batch entry — packing,
// the slab of frames and its release, the frame pool, every failure path — under ASan/UBSan/LSan and TSan. Test infrastructure
// (tests/test_track_frames_cpu.py); nothing here is part of the product.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dsdtm_amd.h"
#include "driver_check.h"
#include "fake_hip.h"

static const int W = 64, H = 48, L = 3, NF = 5;

// One tracker's inputs: a reference frame with n features and a local map of M points observed by one keyframe.
struct Tracker {
    std::vector<uint8_t> img;
    dsdtm_frame *ref = nullptr, *k0 = nullptr;
    const dsdtm_frame* kf[1];
    int n, M;
    std::vector<float> px, opx;
    std::vector<double> be, pw, mpw, ob, Tk;
    std::vector<uint8_t> ini, bad, mask;
    std::vector<int32_t> found, off, okf, olv;
    double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    dsdtm_track_desc d{};
    bool init(dsdtm_ctx* ctx, int n_, int M_, bool with_mask) {
        n = n_; M = M_;
        img.assign((size_t)W * H, (uint8_t)(5 + n));
        if (dsdtm_frame_create_from_image(ctx, img.data(), W, H, W, L, &ref) != DSDTM_OK) return false;
        if (dsdtm_frame_create_from_image(ctx, img.data(), W, H, W, L, &k0) != DSDTM_OK) return false;
        kf[0] = k0;
        px.assign(2 * (size_t)n + 2, 1.f); opx.assign(2 * (size_t)M + 2, 1.f);
        be.assign(3 * (size_t)n + 3, 0.0); pw.assign(3 * (size_t)n + 3, 0.0); mpw.assign(3 * (size_t)M + 3, 0.0); ob.assign(3 * (size_t)M + 3, 0.0);
        Tk.assign(12, 0.0);
        ini.assign((size_t)n + 1, 1); bad.assign((size_t)M + 1, 0); found.assign((size_t)M + 1, 2); okf.assign((size_t)M + 1, 0); olv.assign((size_t)M + 1, 0);
        off.resize((size_t)M + 1);
        for (int i = 0; i <= M; ++i) off[(size_t)i] = i;
        mask.assign((size_t)W * H, 255);
        d.image = img.data(); d.width = W; d.height = H; d.stride = W; d.levels = L;
        d.ref = ref; d.n_ref_features = n; d.ref_px_xy = px.data(); d.ref_bearing = be.data(); d.ref_p_world = pw.data(); d.ref_initial = ini.data();
        d.T_ref_w = T; d.T_seed = T; d.align = dsdtm_align_params{L, 0, 10, 15}; d.min_tracked = 0;
        d.kf = kf; d.n_kf = 1; d.T_kf_w = Tk.data(); d.n_points = M;
        d.mp_world = mpw.data(); d.mp_found = found.data(); d.mp_bad = bad.data(); d.obs_offset = off.data();
        d.obs_kf = okf.data(); d.obs_px = opx.data(); d.obs_level = olv.data(); d.obs_bearing = ob.data();
        if (with_mask) { d.mask = mask.data(); d.mask_stride = W; }
        d.cell_size = 8; d.max_pyr_levels = L + 1; d.max_matches = 200; d.align2d_iters = 10; d.pose_opt.max_iterations = 100;
        return true;
    }
    void release(dsdtm_ctx* ctx) { dsdtm_frame_destroy(ctx, ref); dsdtm_frame_destroy(ctx, k0); }
};

struct Batch {
    std::vector<Tracker> t;
    std::vector<dsdtm_track_desc> d;
    std::vector<dsdtm_track_result> r;
    std::vector<dsdtm_track_match> ms;
    std::vector<double> rn;
    std::vector<uint8_t> grid;
    bool init(dsdtm_ctx* ctx) {
        // feature counts over four register bands and a frame that Run skips (Min_fts); an empty map; a mask
        const int n[NF] = {40, 150, 300, 600, 10}, M[NF] = {50, 0, 30, 70, 20};
        t.resize(NF);
        for (int f = 0; f < NF; ++f)
            if (!t[(size_t)f].init(ctx, n[f], M[f], f == 2)) return false;
        d.clear();
        for (auto& x : t) d.push_back(x.d);
        r.assign(NF, dsdtm_track_result{});
        ms.assign((size_t)NF * 200, dsdtm_track_match{});
        rn.assign((size_t)NF * 200, 0.0);
        grid.assign(200, 7);
        return true;
    }
    int run(dsdtm_ctx* ctx) {
        const dsdtm_camera cam{60.f, 60.f, 32.f, 24.f, 60.f, W, H};
        return dsdtm_track_frames(ctx, &cam, NF, d.data(), r.data(), ms.data(), rn.data(), grid.data());
    }
    bool none_out() const { for (const auto& x : r) if (x.frame) return false; return true; }
    void destroy_shuffled(dsdtm_ctx* ctx, unsigned seed) {
        std::vector<int> o(NF);
        for (int i = 0; i < NF; ++i) o[(size_t)i] = i;
        std::shuffle(o.begin(), o.end(), std::mt19937(seed));
        for (int i : o) { dsdtm_frame_destroy(ctx, r[(size_t)i].frame); r[(size_t)i].frame = nullptr; }
    }
    void release(dsdtm_ctx* ctx) { for (auto& x : t) x.release(ctx); }
};

// every launch and copy of the call fails once: an error, no frame handed out, nothing pending; the context stays usable and the
// frames of a successful call are destroyed in random order
static bool batch_failures() {
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    Batch b;
    CHECK(b.init(ctx));
    CHECK(b.run(ctx) == DSDTM_OK);
    for (int f = 0; f < NF; ++f) CHECK(b.r[(size_t)f].frame != nullptr && b.r[(size_t)f].n_tracked == (f == 4 ? 0 : b.t[(size_t)f].n));
    b.destroy_shuffled(ctx, 1);
    const size_t live0 = fake_hip_live_allocations();
    const char* points[] = {"ingest_launch", "pyrdown_launch", "sparse_align_launch", "hipMemcpyAsync", "hipStreamSynchronize",
                            "track_match_launch", "track_replay_launch", "pose_opt_launch", "hipMalloc", "hipHostGetDevicePointer"};
    for (const char* api : points) {
        for (long nth = 1; nth <= 4; ++nth) {
            fake_hip_fail(api, nth);
            const int rc = b.run(ctx);
            fake_hip_fail(api, 0);
            if (rc == DSDTM_OK) { b.destroy_shuffled(ctx, (unsigned)nth); continue; }    // (fewer than nth calls of this api)
            CHECK(b.none_out() && fake_hip_pending() == 0);
            CHECK(b.run(ctx) == DSDTM_OK && !b.none_out());                               // and the context is usable
            b.destroy_shuffled(ctx, (unsigned)nth + 7);
        }
    }
    CHECK(fake_hip_live_allocations() <= live0 + 2);   // (the pool may keep the slab and the staging may have grown)
    // invalid: a shared field differs in frame 3; observations out of range in frame 2; a foreign reference frame
    {
        Batch c;
        CHECK(c.init(ctx));
        c.d[3].cell_size = 9;
        CHECK(c.run(ctx) == DSDTM_ERR_INVALID && c.none_out() && strstr(dsdtm_last_error(ctx), "frame 3") != nullptr);
        c.d[3].cell_size = 8;
        c.t[2].okf[0] = 5;
        CHECK(c.run(ctx) == DSDTM_ERR_INVALID && c.none_out() && strstr(dsdtm_last_error(ctx), "frame 2") != nullptr);
        c.t[2].okf[0] = 0;
        dsdtm_ctx* other = nullptr;
        CHECK(dsdtm_create(0, &other) == DSDTM_OK);
        dsdtm_frame* foreign = nullptr;
        CHECK(dsdtm_frame_create_from_image(other, c.t[0].img.data(), W, H, W, L, &foreign) == DSDTM_OK);
        c.d[1].ref = foreign;
        CHECK(c.run(ctx) == DSDTM_ERR_INVALID && c.none_out());
        c.d[1].ref = c.t[1].ref;
        c.d[4].n_ref_features = 705;
        CHECK(c.run(ctx) == DSDTM_ERR_INVALID && c.none_out());
        c.d[4].n_ref_features = c.t[4].n;
        CHECK(c.run(ctx) == DSDTM_OK && !c.none_out());
        // the new frames as reference and keyframe of a single call
        dsdtm_track_desc one = c.d[0];
        one.ref = c.r[1].frame;
        const dsdtm_frame* kf1[1] = {c.r[2].frame};
        one.kf = kf1;
        dsdtm_track_result r1{};
        CHECK(dsdtm_track_frame(ctx, &(const dsdtm_camera&)dsdtm_camera{60.f, 60.f, 32.f, 24.f, 60.f, W, H}, &one, &r1, c.ms.data(), c.rn.data()) == DSDTM_OK);
        dsdtm_frame_destroy(ctx, r1.frame);
        dsdtm_frame_destroy(other, foreign);
        dsdtm_destroy(other);
        c.release(ctx);
        // frames destroyed after their context: freed, not pooled
        dsdtm_track_result keep[NF];
        memcpy(keep, c.r.data(), sizeof keep);
        b.release(ctx);
        dsdtm_destroy(ctx);
        for (int i = NF - 1; i >= 0; --i) dsdtm_frame_destroy(ctx, keep[i].frame);
    }
    CHECK(fake_hip_errors().empty());
    return true;
}

// every way an image can arrive, in one call (dsdtm_track_frames routes each frame's image on its own): level 0 of every frame must
// reach its slot of the slab, and Run's range must reach the device exactly once — with the first slot's ingest launch, or with a
// launch of its own where the first slot travels by the copy engine
enum Arrival { DEV_STRIDED, PAGEABLE, PAGEABLE_STRIDED, PINNED, PINNED_ODD, DEV };
struct FrameHead { void* owner; int device; uint8_t* d; };      // the first members of dsdtm_frame (api_internal.h asserts their layout)
static uint8_t pixel(int f, int x, int y) { return (uint8_t)(x * 3 + y * 7 + f * 31 + 1); }
struct Arrivals {
    int nf = 0;
    std::vector<Tracker> t;
    std::vector<dsdtm_track_desc> d;
    std::vector<dsdtm_track_result> r;
    std::vector<dsdtm_track_match> ms;
    std::vector<double> rn;
    std::vector<std::vector<uint8_t>> pageable;
    std::vector<std::pair<void*, bool>> owned;      // (allocation, pinned)
    bool init(dsdtm_ctx* ctx, const std::vector<Arrival>& how, const std::vector<int>& n) {
        nf = (int)how.size();
        t.resize((size_t)nf);
        pageable.resize((size_t)nf);
        for (int f = 0; f < nf; ++f) {
            if (!t[(size_t)f].init(ctx, n[(size_t)f], 20, false)) return false;
            const Arrival a = how[(size_t)f];
            const int stride = (a == DEV_STRIDED || a == PAGEABLE_STRIDED) ? W + 16 : W;
            const size_t bytes = (size_t)stride * H + 16;
            void* base = nullptr;
            if (a == DEV_STRIDED || a == DEV) { if (hipMalloc(&base, bytes) != hipSuccess) return false; owned.emplace_back(base, false); }
            else if (a == PINNED || a == PINNED_ODD) { if (hipHostMalloc(&base, bytes, 0) != hipSuccess) return false; owned.emplace_back(base, true); }
            else { pageable[(size_t)f].assign(bytes, 0); base = pageable[(size_t)f].data(); }
            uint8_t* im = (uint8_t*)base + (a == PINNED_ODD ? 4 : 0);
            memset(base, 0xEE, bytes);
            for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) im[(size_t)y * stride + x] = pixel(f, x, y);
            t[(size_t)f].d.image = im; t[(size_t)f].d.stride = stride;
            d.push_back(t[(size_t)f].d);
        }
        r.assign((size_t)nf, dsdtm_track_result{});
        ms.assign((size_t)nf * 200, dsdtm_track_match{});
        rn.assign((size_t)nf * 200, 0.0);
        return true;
    }
    int run(dsdtm_ctx* ctx) {
        const dsdtm_camera cam{60.f, 60.f, 32.f, 24.f, 60.f, W, H};
        return dsdtm_track_frames(ctx, &cam, nf, d.data(), r.data(), ms.data(), rn.data(), nullptr);
    }
    bool none_out() const { for (const auto& x : r) if (x.frame) return false; return true; }
    bool arrived() const {
        for (int f = 0; f < nf; ++f) {
            CHECK(r[(size_t)f].frame != nullptr && r[(size_t)f].n_tracked == t[(size_t)f].n);       // (Run read its range on the device)
            const uint8_t* l0 = ((const FrameHead*)r[(size_t)f].frame)->d;
            for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) CHECK(l0[(size_t)y * W + x] == pixel(f, x, y));
        }
        return true;
    }
    void destroy(dsdtm_ctx* ctx) { for (auto& x : r) { dsdtm_frame_destroy(ctx, x.frame); x.frame = nullptr; } }
    void release(dsdtm_ctx* ctx) {
        for (auto& x : t) x.release(ctx);
        for (auto& o : owned) { if (o.second) (void)hipHostFree(o.first); else (void)hipFree(o.first); }
    }
};
struct CallCounts { long copy2d, copy, ingest; };
static CallCounts counts_now() { return CallCounts{fake_hip_calls("hipMemcpy2DAsync"), fake_hip_calls("hipMemcpyAsync"), fake_hip_calls("ingest_launch")}; }

static bool batch_image_arrivals() {
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    // (a) frame 0 has the fewest features: it stays in slot 0 behind the sort by register band, and it travels by the copy engine
    Arrivals a;
    CHECK(a.init(ctx, {DEV_STRIDED, PAGEABLE, PAGEABLE_STRIDED, PINNED, PINNED_ODD, DEV}, {40, 150, 300, 600, 150, 60}));
    CallCounts c0 = counts_now();
    CHECK(a.run(ctx) == DSDTM_OK && a.arrived());
    CallCounts c1 = counts_now();
    // one 2-D copy (frame 0); the pinned image at an odd address, the local maps, Run's outputs; four images through the ingest
    // kernel and ONE launch more for Run's range, because slot 0 came by the copy engine
    CHECK(c1.copy2d - c0.copy2d == 1 && c1.copy - c0.copy == 3 && c1.ingest - c0.ingest == 4 + 1);
    a.destroy(ctx);
    // (b) two frames, both by the copy engine: no image goes through the ingest kernel, Run's range alone does — once
    Arrivals b;
    CHECK(b.init(ctx, {DEV_STRIDED, PINNED_ODD}, {40, 150}));
    c0 = counts_now();
    CHECK(b.run(ctx) == DSDTM_OK && b.arrived());
    c1 = counts_now();
    CHECK(c1.copy2d - c0.copy2d == 1 && c1.copy - c0.copy == 3 && c1.ingest - c0.ingest == 0 + 1);
    b.destroy(ctx);
    b.release(ctx);
    // every HIP call of (a) fails once: an error, no frame handed out, nothing pending; then the call works and the images arrive
    // (a pinned image whose device alias cannot be had is no error: it travels by the copy engine)
    const char* points[] = {"ingest_launch", "pyrdown_launch", "sparse_align_launch", "hipMemcpyAsync", "hipMemcpy2DAsync", "hipStreamSynchronize",
                            "track_match_launch", "track_replay_launch", "pose_opt_launch", "hipMalloc", "hipHostGetDevicePointer"};
    for (const char* api : points) {
        for (long nth = 1; nth <= 6; ++nth) {
            fake_hip_fail(api, nth);
            const int rc = a.run(ctx);
            fake_hip_fail(api, 0);
            if (rc == DSDTM_OK) { CHECK(a.arrived()); a.destroy(ctx); continue; }    // (fewer than nth calls of this api, or not an error)
            CHECK(a.none_out() && fake_hip_pending() == 0);
            CHECK(a.run(ctx) == DSDTM_OK && a.arrived());
            a.destroy(ctx);
        }
    }
    a.release(ctx);
    dsdtm_destroy(ctx);
    CHECK(fake_hip_errors().empty());
    return true;
}

// two contexts on two threads, each running batches and destroying their frames (TSan)
static bool two_contexts_two_threads() {
    bool ok[2] = {false, false};
    auto work = [&](int k) {
        dsdtm_ctx* ctx = nullptr;
        if (dsdtm_create(0, &ctx) != DSDTM_OK) return;
        Batch b;
        if (!b.init(ctx)) return;
        bool good = true;
        for (int i = 0; i < 6 && good; ++i) {
            good = b.run(ctx) == DSDTM_OK && !b.none_out();
            b.destroy_shuffled(ctx, (unsigned)(i + 10 * k));
        }
        b.release(ctx);
        dsdtm_destroy(ctx);
        ok[k] = good;
    };
    std::thread t0(work, 0), t1(work, 1);
    t0.join(); t1.join();
    CHECK(ok[0] && ok[1]);
    CHECK(fake_hip_errors().empty());
    return true;
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"batch_failures", batch_failures}, {"batch_image_arrivals", batch_image_arrivals},
                                                                {"two_contexts_two_threads", two_contexts_two_threads}};
    int failed = 0, n_named = 0;
    bool trace = false;                                // --trace: the call trace behind every scenario (fake_hip_print_trace)
    for (int i = 1; i < argc; ++i) { if (std::string(argv[i]) == "--trace") trace = true; else n_named += 1; }
    for (const auto& sc : all) {
        bool wanted = n_named == 0;
        for (int i = 1; i < argc; ++i) wanted = wanted || sc.first == argv[i];
        if (!wanted) continue;
        fake_hip_reset();
        if (trace) std::printf("== %s\n", sc.first.c_str());
        const bool ok = sc.second();
        if (trace) fake_hip_print_trace(stdout);      // (what the scenario left behind its last reset)
        std::printf("%s %s\n", ok ? "ok" : "FAILED", sc.first.c_str());
        std::fflush(stdout);
        failed += ok ? 0 : 1;
    }
    return failed ? 1 : 0;
}
