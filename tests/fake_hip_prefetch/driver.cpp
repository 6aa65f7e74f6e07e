// dsdtm_frame_prefetch / dsdtm_frame_wait / dsdtm_track_frame_on / dsdtm_frame_lift against the fake HIP runtime of
// tests/fake_hip (unmodified) and the faked rgbd.hip launches beside this file: the host side of the prefetch path — the
// staging ring, the frame pool with pending buffers, every failure path, teardown with a prefetch pending — under
// ASan/UBSan/LSan and TSan. Test infrastructure (tests/test_frame_prefetch_cpu.py); nothing here is part of the product.
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dsdtm_amd.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_rgbd.h"

static const int W = 64, H = 48, L = 3;
static const dsdtm_camera CAM = {500.f, 500.f, 32.f, 24.f, 500.f, W, H};
static const double EYE[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

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
    void scribble() { std::fill(gray.begin(), gray.end(), 0xFF); std::fill(depth.begin(), depth.end(), 0xFFFF); }
};

// the frame's depth plane, through the lift: the raw values of the map the frame was made from (the faked launches keep them)
static bool plane_is(dsdtm_ctx* ctx, const dsdtm_frame* f, int tag) {
    float px[8] = {0.f, 0.f, 5.f, 7.f, (float)(W - 1), (float)(H - 1), 31.f, 20.f};
    float d[4];
    double p[12];
    if (dsdtm_frame_lift(ctx, f, &CAM, EYE, px, 4, d, p) != DSDTM_OK) return false;
    for (int i = 0; i < 4; ++i)
        if (d[i] != (float)(tag * 100 + (int)px[2 * i])) { std::fprintf(stderr, "plane of frame %d: pixel %d holds %g\n", tag, i, (double)d[i]); return false; }
    return true;
}

// ---- every launch or copy of dsdtm_frame_prefetch failing once -----------------------------------------------------------
static bool prefetch_failures() {
    fake_hip_reset();
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    {   // a first prefetch creates the stream, the events and the ring: each of those failing
        const char* first[] = {"hipStreamCreateWithFlags", "hipEventCreateWithFlags", "hipHostMalloc", "hipMalloc"};
        for (const char* api : first) {
            Images a(1);
            dsdtm_frame* f = (dsdtm_frame*)1;
            fake_hip_fail(api, 1);
            const int rc = dsdtm_frame_prefetch(ctx, &a.im, &f);
            CHECK(rc == DSDTM_ERR_HIP || rc == DSDTM_ERR_NOMEM);
            CHECK(f == nullptr && fake_hip_pending() == 0);
            CHECK(std::strlen(dsdtm_last_error(ctx)) > 0);
        }
    }
    // pinned memory of the caller (read in place): at an odd address the gray image goes through the copy engine
    void* pin = nullptr;
    CHECK(hipHostMalloc(&pin, (size_t)W * H + 64, 0) == hipSuccess);
    std::memset(pin, 9, (size_t)W * H + 64);
    void* dev = nullptr;
    CHECK(hipMalloc(&dev, (size_t)(W + 8) * H) == hipSuccess);
    struct Case { const char* api; int source; };   // source 0: pageable, 1: pinned at an odd address, 2: device, row-strided
    const Case cases[] = {{"hipHostGetDevicePointer", 0}, {"ingest_launch", 0}, {"pyrdown_launch", 0}, {"depth", 0}, {"hipEventRecord", 0},
                          {"hipMemcpyAsync", 1}, {"hipMemcpy2DAsync", 2}};
    int tag = 2;
    for (const Case& c : cases) {
        Images a(tag);
        if (c.source == 1) a.im.gray = (const uint8_t*)pin + 4;
        if (c.source == 2) { a.im.gray = (const uint8_t*)dev; a.im.stride = W + 8; }
        dsdtm_frame* f = (dsdtm_frame*)1;
        const size_t live = fake_hip_live_allocations();
        if (std::strcmp(c.api, "depth") == 0) fake_rgbd_fail(1, 0); else fake_hip_fail(c.api, 1);
        CHECK(dsdtm_frame_prefetch(ctx, &a.im, &f) == DSDTM_ERR_HIP);
        CHECK(f == nullptr);                              // no frame handed out
        CHECK(fake_hip_pending() == 0);                   // nothing pending: what had been enqueued was waited for
        CHECK(fake_hip_live_allocations() <= live + 1);   // (a buffer may have gone to the pool; none is lost: the leak check at exit)
        a.scribble();
        // and a later prefetch works, on the same kind of source
        Images b(tag + 1);
        if (c.source == 1) b.im.gray = (const uint8_t*)pin + 4;
        if (c.source == 2) { b.im.gray = (const uint8_t*)dev; b.im.stride = W + 8; }
        CHECK(dsdtm_frame_prefetch(ctx, &b.im, &f) == DSDTM_OK && f != nullptr);
        b.scribble();
        CHECK(fake_hip_pending() > 0);                    // it returned at once: nothing has run yet
        CHECK(plane_is(ctx, f, tag + 1));
        CHECK(dsdtm_frame_wait(ctx, f) == DSDTM_OK);
        dsdtm_frame_destroy(ctx, f);
        tag += 2;
    }
    {   // the lift's own launch failing leaves the context usable
        Images a(40);
        dsdtm_frame* f = nullptr;
        CHECK(dsdtm_frame_prefetch(ctx, &a.im, &f) == DSDTM_OK);
        float px[2] = {1.f, 1.f}, d[1]; double p[3];
        fake_rgbd_fail(0, 1);
        CHECK(dsdtm_frame_lift(ctx, f, &CAM, EYE, px, 1, d, p) == DSDTM_ERR_HIP);
        CHECK(plane_is(ctx, f, 40));
        dsdtm_frame_destroy(ctx, f);
    }
    CHECK(fake_hip_errors().empty());
    dsdtm_destroy(ctx);
    CHECK(hipFree(dev) == hipSuccess && hipHostFree(pin) == hipSuccess);
    CHECK(fake_hip_live_allocations() == 0);              // everything the context owned is gone
    return true;
}

// ---- the ring: a slot is written again only after the frame that used it is resident ----------------------------------------
static bool ring_slot_reuse() {
    fake_hip_reset();
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    Images a(1), b(2), c(3);
    dsdtm_frame *fa = nullptr, *fb = nullptr, *fc = nullptr;
    CHECK(dsdtm_frame_prefetch(ctx, &a.im, &fa) == DSDTM_OK); a.scribble();
    CHECK(dsdtm_frame_prefetch(ctx, &b.im, &fb) == DSDTM_OK); b.scribble();
    const long waits = fake_hip_calls("hipEventSynchronize");
    const size_t pending = fake_hip_pending();
    CHECK(pending > 0 && fake_hip_log().empty());        // two frames enqueued, nothing has run
    // the third frame takes the first one's slot: the host waits for the first frame's event BEFORE it writes the slot
    CHECK(dsdtm_frame_prefetch(ctx, &c.im, &fc) == DSDTM_OK); c.scribble();
    CHECK(fake_hip_calls("hipEventSynchronize") == waits + 1);
    {
        const std::vector<fake_launch> log = fake_hip_log();
        CHECK(!log.empty() && log[0].name == "ingest");  // frame 1's kernels ran inside that wait ...
        size_t ingests = 0;
        for (const fake_launch& l : log) ingests += l.name == "ingest";
        CHECK(ingests == 1);                              // ... and only frame 1's: frames 2 and 3 are still queued
    }
    // had the slot been written first, frame 1's plane would hold frame 3's values
    CHECK(plane_is(ctx, fa, 1) && plane_is(ctx, fc, 3) && plane_is(ctx, fb, 2));
    // settled frames cost nothing more: no further stream waits
    const long sw = fake_hip_calls("hipStreamWaitEvent");
    CHECK(plane_is(ctx, fa, 1) && plane_is(ctx, fb, 2) && plane_is(ctx, fc, 3));
    CHECK(fake_hip_calls("hipStreamWaitEvent") == sw);
    CHECK(dsdtm_frame_wait(ctx, fc) == DSDTM_OK && fake_hip_calls("hipEventSynchronize") == waits + 1);
    dsdtm_frame_destroy(ctx, fa); dsdtm_frame_destroy(ctx, fb); dsdtm_frame_destroy(ctx, fc);
    CHECK(fake_hip_errors().empty());
    dsdtm_destroy(ctx);
    CHECK(fake_hip_live_allocations() == 0);
    return true;
}

// ---- the pool: a pending frame's buffer goes to the pool with its event; the next user's stream waits for it --------------
static bool pooled_pending_buffer() {
    fake_hip_reset();
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    Images a(1, false), b(2, false);
    dsdtm_frame *fa = nullptr, *fb = nullptr;
    CHECK(dsdtm_frame_create_from_image(ctx, b.gray.data(), W, H, W, L, &fb) == DSDTM_OK);   // (warm-up: the context's staging blocks exist)
    dsdtm_frame_destroy(ctx, fb);
    fb = nullptr;
    fake_hip_reset();
    CHECK(dsdtm_frame_prefetch(ctx, &a.im, &fa) == DSDTM_OK);
    const size_t live = fake_hip_live_allocations();
    dsdtm_frame_destroy(ctx, fa);                         // pending: legal, and no wait
    CHECK(fake_hip_pending() > 0 && fake_hip_live_allocations() == live);
    const long sw = fake_hip_calls("hipStreamWaitEvent");
    CHECK(dsdtm_frame_create_from_image(ctx, b.gray.data(), W, H, W, L, &fb) == DSDTM_OK);
    CHECK(fake_hip_live_allocations() == live);           // the pooled buffer was taken ...
    CHECK(fake_hip_calls("hipStreamWaitEvent") == sw + 1);   // ... and the compute stream waited for the event behind it
    {
        // execution order: the destroyed frame's prefetch first, then the new frame's kernels into the same buffer
        const std::vector<fake_launch> log = fake_hip_log();
        std::vector<const fake_launch*> ing;
        for (const fake_launch& l : log) if (l.name == "ingest") ing.push_back(&l);
        CHECK(ing.size() == 2 && ing[0]->stream != ing[1]->stream && ing[0]->seq < ing[1]->seq);
        size_t first_pyr_of_b = 0, last_pyr_of_a = 0;
        for (size_t i = 0; i < log.size(); ++i) {
            if (log[i].name != "pyrdown") continue;
            if (log[i].stream == ing[0]->stream) last_pyr_of_a = i; else if (!first_pyr_of_b) first_pyr_of_b = i;
        }
        CHECK(last_pyr_of_a < first_pyr_of_b);
    }
    // a prefetch that takes a pooled pending buffer runs on the same stream: in order without a wait
    Images c(3, false), d(4, false);
    dsdtm_frame *fc = nullptr, *fd = nullptr;
    CHECK(dsdtm_frame_prefetch(ctx, &c.im, &fc) == DSDTM_OK);
    dsdtm_frame_destroy(ctx, fc);
    const long sw2 = fake_hip_calls("hipStreamWaitEvent");
    CHECK(dsdtm_frame_prefetch(ctx, &d.im, &fd) == DSDTM_OK);
    CHECK(fake_hip_calls("hipStreamWaitEvent") == sw2);
    dsdtm_frame_destroy(ctx, fb); dsdtm_frame_destroy(ctx, fd);
    CHECK(fake_hip_errors().empty());
    dsdtm_destroy(ctx);
    CHECK(fake_hip_live_allocations() == 0);
    return true;
}

// ---- dsdtm_destroy with a prefetch pending --------------------------------------------------------------------------------
static bool destroy_with_a_prefetch_pending() {
    fake_hip_reset();
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    Images a(1), b(2);
    dsdtm_frame *fa = nullptr, *fb = nullptr;
    CHECK(dsdtm_frame_prefetch(ctx, &a.im, &fa) == DSDTM_OK);
    CHECK(dsdtm_frame_prefetch(ctx, &b.im, &fb) == DSDTM_OK);
    dsdtm_frame_destroy(ctx, fb);                         // one pending buffer in the pool, one pending frame alive
    CHECK(fake_hip_pending() > 0);
    dsdtm_destroy(ctx);                                   // waits for the prefetch stream before it frees the ring and the pool
    CHECK(fake_hip_pending() == 0);
    dsdtm_frame_destroy(ctx, fa);                         // the context is gone: the pointer is compared only, the buffer freed
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// ---- prefetch(k + 1); track_frame_on(k) ------------------------------------------------------------------------------------
struct Seq {
    std::vector<float> px;
    std::vector<double> be, pw;
    std::vector<uint8_t> ini;
    dsdtm_track_desc d{};
    dsdtm_track_result r{};
    std::vector<dsdtm_track_match> ms;
    std::vector<double> rn;
    explicit Seq(int n) : px(2 * (size_t)n, 1.f), be(3 * (size_t)n, 0.0), pw(3 * (size_t)n, 0.0), ini((size_t)n, 1), ms(200), rn(200) {
        d.width = W; d.height = H; d.stride = W; d.levels = L;
        d.n_ref_features = n; d.ref_px_xy = px.data(); d.ref_bearing = be.data(); d.ref_p_world = pw.data(); d.ref_initial = ini.data();
        d.T_ref_w = EYE; d.T_seed = EYE; d.align = dsdtm_align_params{L, 0, 10, 15}; d.min_tracked = 0;
        d.cell_size = 8; d.max_pyr_levels = L + 1; d.max_matches = 200; d.align2d_iters = 10; d.pose_opt.max_iterations = 100;
    }
};

static bool tracked_sequence(int frames) {
    dsdtm_ctx* ctx = nullptr;
    CHECK(dsdtm_create(0, &ctx) == DSDTM_OK);
    Seq s(40);
    Images first(1);
    dsdtm_frame* last = nullptr;
    CHECK(dsdtm_frame_create_from_image(ctx, first.gray.data(), W, H, W, L, &last) == DSDTM_OK);
    dsdtm_frame* next = nullptr;
    {
        Images im(2);
        CHECK(dsdtm_frame_prefetch(ctx, &im.im, &next) == DSDTM_OK);
        im.scribble();
    }                                                     // (the staged images are gone when the block ends)
    for (int k = 0; k < frames; ++k) {
        dsdtm_frame* cur = next;
        next = nullptr;
        if (k + 1 < frames) {
            Images im(3 + k);
            CHECK(dsdtm_frame_prefetch(ctx, &im.im, &next) == DSDTM_OK);
            im.scribble();
        }
        s.d.ref = last;
        s.d.image = first.gray.data();
        CHECK(dsdtm_track_frame_on(ctx, &CAM, &s.d, cur, &s.r, s.ms.data(), s.rn.data()) == DSDTM_ERR_INVALID);   // image must be NULL
        s.d.image = nullptr;
        CHECK(dsdtm_track_frame_on(ctx, &CAM, &s.d, cur, &s.r, s.ms.data(), s.rn.data()) == DSDTM_OK);
        CHECK(s.r.frame == cur && s.r.n_tracked == 40);
        CHECK(plane_is(ctx, cur, 2 + k));
        dsdtm_frame_destroy(ctx, last);
        last = cur;
    }
    dsdtm_frame_destroy(ctx, last);
    dsdtm_destroy(ctx);
    return true;
}

static bool prefetch_then_track() {
    fake_hip_reset();
    CHECK(tracked_sequence(5));
    CHECK(fake_hip_errors().empty() && fake_hip_live_allocations() == 0);
    return true;
}

static bool two_contexts_two_threads() {
    fake_hip_reset();
    bool ok[2] = {false, false};
    std::thread t0([&] { ok[0] = tracked_sequence(6); });
    std::thread t1([&] { ok[1] = tracked_sequence(4); });
    t0.join(); t1.join();
    CHECK(ok[0] && ok[1]);
    CHECK(fake_hip_errors().empty() && fake_hip_live_allocations() == 0);
    return true;
}

int main(int argc, char** argv) {
    struct { const char* name; bool (*fn)(); } tests[] = {
        {"prefetch_failures", prefetch_failures}, {"ring_slot_reuse", ring_slot_reuse}, {"pooled_pending_buffer", pooled_pending_buffer},
        {"destroy_with_a_prefetch_pending", destroy_with_a_prefetch_pending}, {"prefetch_then_track", prefetch_then_track},
        {"two_contexts_two_threads", two_contexts_two_threads}};
    int failed = 0;
    bool trace = false;                                // --trace: the call trace behind every scenario (fake_hip_print_trace)
    const char* only = nullptr;
    for (int i = 1; i < argc; ++i) { if (std::string(argv[i]) == "--trace") trace = true; else if (!only) only = argv[i]; }
    for (auto& t : tests) {
        if (only && std::string(only) != t.name) continue;
        fake_hip_reset();
        if (trace) std::printf("== %s\n", t.name);
        const bool ok = t.fn();
        if (trace) fake_hip_print_trace(stdout);      // (what the scenario left behind its last reset)
        std::printf("%s %s\n", ok ? "ok" : "FAILED", t.name);
        std::fflush(stdout);
        failed += !ok;
    }
    return failed ? 1 : 0;
}
