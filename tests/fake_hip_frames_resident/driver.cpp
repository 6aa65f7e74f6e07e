// dsdtm_track_frames on RESIDENT frames (descs[f].image == NULL, results[f].frame names the frame) against the fake HIP runtime of
// tests/fake_hip (unmodified) and the faked rgbd.hip launches of tests/fake_hip_prefetch: the host side of the resident mode —
// ownership of the frames on success and on every failure, the argument checks, no slab, the device-side wait for pending
// prefetches, teardown — under ASan/UBSan/LSan and TSan. Test infrastructure (tests/test_track_frames_resident_cpu.py); nothing
// here is part of the product.
// (The fake Run kernel models the PACKED layout — it touches cur_pyr over n_pairs * pitch — so the batches here keep ONE frame per
// register band: a launch of one pair, whose packed range is the frame itself.)
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dsdtm_amd.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_rgbd.h"

static const int W = 64, H = 48, L = 3, NF = 7;
static const dsdtm_camera CAM = {60.f, 60.f, 32.f, 24.f, 60.f, W, H};
static const double EYE[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
// one frame per register band (<= 128, 192, 256, 320, 448, 704) and one that Run skips (Min_fts)
static const int N_REF[NF] = {40, 150, 230, 300, 400, 600, 10}, N_PTS[NF] = {50, 0, 30, 70, 20, 16, 5};

// a frame's images in pageable memory (staged by the prefetch): gray all `tag`, depth tag * 100 + column
struct Images {
    std::vector<uint8_t> gray;
    std::vector<uint16_t> depth;
    dsdtm_frame_image im{};
    explicit Images(int tag, bool with_depth = true) : gray((size_t)W * H, (uint8_t)tag), depth((size_t)W * H) {
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) depth[(size_t)y * W + x] = (uint16_t)(tag * 100 + x);
        im.gray = gray.data(); im.width = W; im.height = H; im.stride = W; im.levels = L;
        if (with_depth) { im.depth = depth.data(); im.depth_stride = W; im.depth_scale = 5000.f; }
    }
};

// the frame's depth plane, through the lift (the faked launches keep the raw values of the map the frame was made from)
static bool plane_is(dsdtm_ctx* ctx, const dsdtm_frame* f, int tag) {
    float px[4] = {0.f, 0.f, 31.f, 20.f};
    float d[2];
    double p[6];
    if (dsdtm_frame_lift(ctx, f, &CAM, EYE, px, 2, d, p) != DSDTM_OK) return false;
    return d[0] == (float)(tag * 100) && d[1] == (float)(tag * 100 + 31);
}

// One tracker's inputs: a reference frame with n features and a local map of M points observed by one keyframe.
struct Tracker {
    std::vector<uint8_t> img;
    dsdtm_frame *ref = nullptr, *k0 = nullptr;
    const dsdtm_frame* kf[1];
    int n, M;
    std::vector<float> px, opx;
    std::vector<double> be, pw, mpw, ob, Tk;
    std::vector<uint8_t> ini, bad;
    std::vector<int32_t> found, off, okf, olv;
    dsdtm_track_desc d{};
    bool init(dsdtm_ctx* ctx, int n_, int M_) {
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
        d.image = nullptr; d.width = W; d.height = H; d.stride = W; d.levels = L;
        d.ref = ref; d.n_ref_features = n; d.ref_px_xy = px.data(); d.ref_bearing = be.data(); d.ref_p_world = pw.data(); d.ref_initial = ini.data();
        d.T_ref_w = EYE; d.T_seed = EYE; d.align = dsdtm_align_params{L, 0, 10, 15}; d.min_tracked = 0;
        d.kf = kf; d.n_kf = 1; d.T_kf_w = Tk.data(); d.n_points = M;
        d.mp_world = mpw.data(); d.mp_found = found.data(); d.mp_bad = bad.data(); d.obs_offset = off.data();
        d.obs_kf = okf.data(); d.obs_px = opx.data(); d.obs_level = olv.data(); d.obs_bearing = ob.data();
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
    std::vector<dsdtm_frame*> cur;     // the resident frames of the next call, in the caller's order
    std::vector<int> tag;
    bool init(dsdtm_ctx* ctx) {
        t.resize(NF);
        for (int f = 0; f < NF; ++f)
            if (!t[(size_t)f].init(ctx, N_REF[f], N_PTS[f])) return false;
        d.clear();
        for (auto& x : t) d.push_back(x.d);
        r.assign(NF, dsdtm_track_result{});
        ms.assign((size_t)NF * 200, dsdtm_track_match{});
        rn.assign((size_t)NF * 200, 0.0);
        grid.assign(256, 7);
        cur.assign(NF, nullptr);
        tag.assign(NF, 0);
        return true;
    }
    // one prefetch per tracker, none waited for (every second one with a depth map)
    bool prefetch_all(dsdtm_ctx* ctx, int tag0, bool depth = true) {
        for (int f = 0; f < NF; ++f) {
            Images im(tag0 + f, depth && f % 2 == 0);
            if (dsdtm_frame_prefetch(ctx, &im.im, &cur[(size_t)f]) != DSDTM_OK) return false;
            tag[(size_t)f] = tag0 + f;
        }                                                 // (the staged images are gone here: the ring holds them)
        return true;
    }
    int run(dsdtm_ctx* ctx) {
        for (int f = 0; f < NF; ++f) { r[(size_t)f] = dsdtm_track_result{}; r[(size_t)f].frame = cur[(size_t)f]; }
        return dsdtm_track_frames(ctx, &CAM, NF, d.data(), r.data(), ms.data(), rn.data(), grid.data());
    }
    bool frames_kept() const { for (int f = 0; f < NF; ++f) if (r[(size_t)f].frame != cur[(size_t)f]) return false; return true; }
    bool tracked() const { for (int f = 0; f < NF; ++f) if (r[(size_t)f].n_tracked != (f == NF - 1 ? 0 : N_REF[f])) return false; return true; }
    bool planes(dsdtm_ctx* ctx) const { for (int f = 0; f < NF; f += 2) if (!plane_is(ctx, cur[(size_t)f], tag[(size_t)f])) return false; return true; }
    // every frame of the call through the single entry: it is still a frame of the caller's
    bool track_each_alone(dsdtm_ctx* ctx) {
        for (int f = 0; f < NF; ++f) {
            dsdtm_track_result r1{};
            if (dsdtm_track_frame_on(ctx, &CAM, &d[(size_t)f], cur[(size_t)f], &r1, ms.data(), rn.data()) != DSDTM_OK) return false;
            if (r1.frame != cur[(size_t)f] || r1.n_tracked != (f == NF - 1 ? 0 : N_REF[f])) return false;
        }
        return true;
    }
    void destroy_cur(dsdtm_ctx* ctx) { for (auto& c : cur) { dsdtm_frame_destroy(ctx, c); c = nullptr; } }
    void release(dsdtm_ctx* ctx) { for (auto& x : t) x.release(ctx); }
};

// ---- a resident call on pending frames: ordered behind the prefetches on the device, no slab, the frames stay the caller's ----
static bool resident_call() {
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    Batch b;
    CHECK(b.init(ctx));
    CHECK(b.prefetch_all(ctx, 1) && b.run(ctx) == DSDTM_OK && b.frames_kept() && b.tracked());    // (warm-up: the staging blocks exist)
    b.destroy_cur(ctx);
    fake_hip_drain_all();
    const size_t log0 = fake_hip_log().size();
    CHECK(b.prefetch_all(ctx, 20));
    CHECK(fake_hip_pending() > 0);                        // (pageable images: the two-slot staging ring lets the last frames stay pending)
    const long mallocs = fake_hip_calls("hipMalloc"), host_waits = fake_hip_calls("hipEventSynchronize"), pyr = fake_hip_calls("pyrdown_launch");
    const size_t live = fake_hip_live_allocations();
    CHECK(b.run(ctx) == DSDTM_OK);
    CHECK(b.frames_kept() && b.tracked());
    CHECK(fake_hip_calls("hipMalloc") == mallocs && fake_hip_live_allocations() == live);         // no slab
    CHECK(fake_hip_calls("hipEventSynchronize") == host_waits);                                   // no host wait on the way in
    CHECK(fake_hip_calls("pyrdown_launch") == pyr);                                               // the chain starts at Run
    {
        // execution order: every prefetch (ingest, pyramid) before the call's first kernel — its own ingest of Run's range
        const std::vector<fake_launch> log = fake_hip_log();
        hipStream_t ps = nullptr;
        long last_prefetch = 0, first_of_call = 0, runs = 0;
        for (size_t i = log0; i < log.size(); ++i) if (log[i].name == "pyrdown") { ps = log[i].stream; last_prefetch = log[i].seq; }
        CHECK(ps != nullptr);
        for (size_t i = log0; i < log.size(); ++i) {
            if (log[i].stream == ps) continue;
            if (!first_of_call) first_of_call = log[i].seq;
            runs += log[i].kind == FAKE_SA_ONE_CU;
        }
        CHECK(first_of_call > last_prefetch && runs == 6);                                        // six bands, one launch each
    }
    CHECK(b.planes(ctx));                                 // the depth maps came through the call
    // settled now: a second call on the same frames (legal: they are the caller's) enqueues no further stream wait
    const long sw = fake_hip_calls("hipStreamWaitEvent");
    CHECK(b.run(ctx) == DSDTM_OK && b.frames_kept() && b.tracked());
    CHECK(fake_hip_calls("hipStreamWaitEvent") == sw);
    // one frame destroyed while the others live; the others as ref / kf of the next call, which runs on frames still pending
    std::vector<dsdtm_frame*> old = b.cur;
    dsdtm_frame_destroy(ctx, old[3]);
    CHECK(b.prefetch_all(ctx, 40));
    const dsdtm_frame* kf1[1] = {old[1]};
    b.d[0].ref = old[2]; b.d[0].kf = kf1;
    CHECK(b.run(ctx) == DSDTM_OK && b.frames_kept() && b.tracked() && b.planes(ctx));
    b.d[0] = b.t[0].d;
    for (int f = 0; f < NF; ++f) if (f != 3) dsdtm_frame_destroy(ctx, old[(size_t)f]);
    b.destroy_cur(ctx);
    b.release(ctx);
    CHECK(fake_hip_errors().empty());
    dsdtm_destroy(ctx);
    CHECK(fake_hip_live_allocations() == 0);
    return true;
}

// ---- every launch or copy of the resident call fails once ------------------------------------------------------------------
static bool resident_failures() {
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    Batch b;
    CHECK(b.init(ctx));
    CHECK(b.prefetch_all(ctx, 1) && b.run(ctx) == DSDTM_OK);
    b.destroy_cur(ctx);
    const char* points[] = {"hipHostGetDevicePointer", "hipSetDevice", "hipStreamWaitEvent", "ingest_launch", "sparse_align_launch",
                            "hipMemcpyAsync", "hipStreamSynchronize", "track_match_launch", "track_replay_launch", "pose_opt_launch"};
    int tag = 10;
    for (const char* api : points) {
        for (long nth = 1; nth <= 3; ++nth) {
            CHECK(b.prefetch_all(ctx, tag));                              // pending: the call is what waits for them
            const size_t live = fake_hip_live_allocations();
            fake_hip_fail(api, nth);
            const int rc = b.run(ctx);
            fake_hip_fail(api, 0);
            CHECK(b.frames_kept());                                       // on success and on every failure
            CHECK(fake_hip_live_allocations() == live);                   // nothing allocated, nothing lost
            if (rc != DSDTM_OK) {
                CHECK(rc == DSDTM_ERR_HIP && std::strlen(dsdtm_last_error(ctx)) > 0);
                // the frames are usable: alone, and in the same call again; their depth maps are theirs
                CHECK(b.track_each_alone(ctx));
                CHECK(b.run(ctx) == DSDTM_OK && b.frames_kept() && b.tracked());
            } else CHECK(b.tracked());                                    // (fewer than nth calls of this api)
            CHECK(b.planes(ctx));
            // the prefetch numbering and the staging ring go on as if nothing had happened: the next step's frames are the next step's
            b.destroy_cur(ctx);
            tag += NF;
            if (tag > 200) tag = 10;
        }
    }
    b.release(ctx);
    CHECK(fake_hip_errors().empty());
    dsdtm_destroy(ctx);
    CHECK(fake_hip_live_allocations() == 0);
    return true;
}

// ---- the argument checks: DSDTM_ERR_INVALID naming frame and field, nothing enqueued, the frames still the caller's --------
static bool resident_arguments() {
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    Batch b;
    CHECK(b.init(ctx));
    CHECK(b.prefetch_all(ctx, 1) && b.run(ctx) == DSDTM_OK);              // (warm-up)
    b.destroy_cur(ctx);
    CHECK(b.prefetch_all(ctx, 30));
    fake_hip_drain_all();
    auto refused = [&](const char* frame, const char* field) {
        const size_t log = fake_hip_log().size(), pending = fake_hip_pending(), live = fake_hip_live_allocations();
        const int rc = b.run(ctx);
        const char* msg = dsdtm_last_error(ctx);
        if (rc != DSDTM_ERR_INVALID || !std::strstr(msg, frame) || !std::strstr(msg, field)) { std::fprintf(stderr, "rc %d: %s (wanted '%s', '%s')\n", rc, msg, frame, field); return false; }
        return fake_hip_log().size() == log && fake_hip_pending() == pending && fake_hip_live_allocations() == live && b.frames_kept();
    };
    std::vector<uint8_t> image((size_t)W * H, 3);
    b.d[4].image = image.data();                                          // a mixture: the first frame that differs is named
    b.d[5].image = image.data();
    CHECK(refused("frame 4", "image"));
    b.d[4].image = nullptr; b.d[5].image = nullptr;
    b.d[0].image = image.data();                                          // (frame 0 decides the mode: frame 1 is the one that differs)
    CHECK(refused("frame 1", "image"));
    b.d[0].image = nullptr;
    dsdtm_frame* keep = b.cur[2];
    b.cur[2] = nullptr;
    CHECK(refused("frame 2", "results[2].frame is NULL"));
    b.cur[2] = b.cur[5];
    CHECK(refused("frame 5", "also frame 2"));                            // the same frame twice
    b.cur[2] = keep;
    b.d[3].ref = b.cur[3];
    CHECK(refused("frame 3", "ref"));                                     // a frame that is its own reference
    b.d[3].ref = b.t[3].ref;
    for (auto& d : b.d) d.width = W + 2;
    CHECK(refused("frame 0", "width"));
    for (auto& d : b.d) { d.width = W; d.height = H - 2; }
    CHECK(refused("frame 0", "height"));
    for (auto& d : b.d) { d.height = H; d.levels = L - 1; d.align.max_level = L - 1; d.max_pyr_levels = L; }
    CHECK(refused("frame 0", "levels"));
    for (int f = 0; f < NF; ++f) b.d[(size_t)f] = b.t[(size_t)f].d;
    b.d[6].levels = L - 1;                                                // (a shared field that differs: named as today)
    CHECK(refused("frame 6", "levels"));
    b.d[6].levels = L;
    {
        dsdtm_ctx* other = nullptr;
        CHECK(dsdtm_create(0, &other) == DSDTM_OK);
        dsdtm_frame* foreign = nullptr;
        CHECK(dsdtm_frame_create_from_image(other, image.data(), W, H, W, L, &foreign) == DSDTM_OK);
        keep = b.cur[1];
        b.cur[1] = foreign;
        CHECK(refused("frame 1", "another context"));
        b.cur[1] = keep;
        dsdtm_frame_destroy(other, foreign);
        dsdtm_destroy(other);
    }
    // a frame from dsdtm_frame_create with levels of its own (not halved): the right size at level 0, refused all the same
    {
        std::vector<uint8_t> l0((size_t)W * H, 1), l1((size_t)(W / 2 - 1) * (H / 2), 1), l2((size_t)(W / 4) * (H / 4), 1);
        dsdtm_pyramid p{};
        p.levels = L;
        p.data[0] = l0.data(); p.width[0] = W; p.height[0] = H; p.stride[0] = W;
        p.data[1] = l1.data(); p.width[1] = W / 2 - 1; p.height[1] = H / 2; p.stride[1] = W / 2 - 1;
        p.data[2] = l2.data(); p.width[2] = W / 4; p.height[2] = H / 4; p.stride[2] = W / 4;
        dsdtm_frame* odd = nullptr;
        CHECK(dsdtm_frame_create(ctx, &p, &odd) == DSDTM_OK);
        keep = b.cur[0];
        b.cur[0] = odd;
        CHECK(refused("frame 0", "levels of results[0].frame"));
        b.cur[0] = keep;
        dsdtm_frame_destroy(ctx, odd);
    }
    // after all that every frame still tracks: alone, then together
    CHECK(b.track_each_alone(ctx));
    CHECK(b.run(ctx) == DSDTM_OK && b.frames_kept() && b.tracked() && b.planes(ctx));
    b.destroy_cur(ctx);
    b.release(ctx);
    CHECK(fake_hip_errors().empty());
    dsdtm_destroy(ctx);
    CHECK(fake_hip_live_allocations() == 0);
    return true;
}

// ---- dsdtm_destroy while the frames of a finished call live on and the next step's are still pending -------------------------
static bool destroy_with_resident_frames() {
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    Batch b;
    CHECK(b.init(ctx));
    CHECK(b.prefetch_all(ctx, 1) && b.run(ctx) == DSDTM_OK && b.frames_kept());
    std::vector<dsdtm_frame*> done = b.cur;
    CHECK(b.prefetch_all(ctx, 20));                       // the next step: pending
    dsdtm_frame_destroy(ctx, b.cur[0]);                   // (one pending buffer in the pool as well)
    b.cur[0] = nullptr;
    CHECK(fake_hip_pending() > 0);
    b.release(ctx);
    dsdtm_destroy(ctx);                                   // waits for the prefetch stream before it frees the ring and the pool
    CHECK(fake_hip_pending() == 0);
    for (dsdtm_frame* f : done) dsdtm_frame_destroy(ctx, f);              // the context is gone: compared only, the buffers freed
    b.destroy_cur(ctx);
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// ---- two contexts on two threads, each in lockstep: prefetch step k + 1, track step k (TSan) ----------------------------------
// (without depth maps: the faked depth launch of tests/fake_hip_prefetch counts its calls in a plain global)
static bool lockstep(int steps) {
    dsdtm_ctx* ctx = nullptr;
    if (dsdtm_create(0, &ctx) != DSDTM_OK) return false;
    Batch b;
    if (!b.init(ctx)) return false;
    bool good = b.prefetch_all(ctx, 1, false);
    for (int k = 0; k < steps && good; ++k) {
        std::vector<dsdtm_frame*> now = b.cur;
        std::vector<int> now_tag = b.tag;
        if (k + 1 < steps) good = b.prefetch_all(ctx, 1 + (k + 1) * NF, false);
        std::vector<dsdtm_frame*> next = b.cur;
        std::vector<int> next_tag = b.tag;
        b.cur = now; b.tag = now_tag;
        good = good && b.run(ctx) == DSDTM_OK && b.frames_kept() && b.tracked();
        b.destroy_cur(ctx);
        b.cur = next; b.tag = next_tag;
        if (k + 1 >= steps) b.cur.assign(NF, nullptr);
    }
    b.release(ctx);
    dsdtm_destroy(ctx);
    return good;
}

static bool two_contexts_two_threads() {
    bool ok[2] = {false, false};
    std::thread t0([&] { ok[0] = lockstep(5); });
    std::thread t1([&] { ok[1] = lockstep(4); });
    t0.join(); t1.join();
    CHECK(ok[0] && ok[1]);
    CHECK(fake_hip_errors().empty() && fake_hip_live_allocations() == 0);
    return true;
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"resident_call", resident_call}, {"resident_failures", resident_failures},
                                                      {"resident_arguments", resident_arguments},
                                                      {"destroy_with_resident_frames", destroy_with_resident_frames},
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
