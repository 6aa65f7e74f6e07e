// libdsdtm_amd_mapping.so's host side (dsdtm_amd/csrc/mapping_api.cpp over trackmap_api_body.h) against the fake HIP runtime of
// tests/fake_hip (unmodified): the checks and the packing of dsdtm_mapping_covisibility, _ba_window and _ba_commit, the event that
// orders the commit behind the solver's stream, every refusal, every failing HIP call, the growth of the staging blocks and the
// memory limit — under ASan/UBSan/LSan. The launches of mapping.hip are the fakes of tests/fake_hip_mapping/fake_mapping.cpp (the
// host functions of dsdtm_mapping_host.hpp), the map's own those of tests/fake_hip_trackmap and tests/fake_hip_localmap. Test
// infrastructure (tests/test_ba_window_fake_hip_cpu.py); nothing here is part of the product.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../dsdtm_amd/host/dsdtm_mapping_host.hpp"
#include "addon_create_failures.h"
#include "driver_check.h"
#include "fake_hip.h"
#include "fake_mapping.h"
#include "fake_trackmap.h"

static const double I12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

static bool named_err(dsdtm_mapping_ctx* ctx, int rc, const char* needle) {
    if (rc != DSDTM_ERR_INVALID || !strstr(dsdtm_mapping_last_error(ctx), needle)) {
        std::fprintf(stderr, "rc %d, error \"%s\", wanted \"%s\"\n", rc, dsdtm_mapping_last_error(ctx), needle);
        return false;
    }
    return true;
}

// A map on the "device" and its mirror on the host: K keyframes of S slots; slot s of keyframe k lists point (k * stride + s) % P and
// observes it unless (k + s) % 5 == 0, so neighbouring keyframes share points.
struct World {
    dsdtm_mapping_ctx* ctx = nullptr;
    dsdtm_trackmap* map = nullptr;
    std::vector<double> p, T, bearing;
    std::vector<uint8_t> bad, observes;
    std::vector<int32_t> found, ns, slots, level;
    std::vector<float> px;
    std::vector<int64_t> off;
    bool open(int K, int S, int P, int stride) {
        CHECK(dsdtm_mapping_create(0, &ctx) == DSDTM_OK && dsdtm_mapping_map_create(ctx, &map) == DSDTM_OK);
        p.resize(3 * (size_t)P); bad.assign((size_t)P, 0); found.assign((size_t)P, 1);
        for (size_t i = 0; i < p.size(); ++i) p[i] = 0.25 * (double)(i % 37);
        CHECK(dsdtm_mapping_points_write(ctx, map, 0, P, p.data(), bad.data(), found.data()) == DSDTM_OK);
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
            CHECK(dsdtm_mapping_keyframe_add(ctx, map, Tk, S, s.data(), o.data(), x.data(), l.data(), b.data(), &got) == DSDTM_OK && got == k);
            off.push_back((int64_t)slots.size()); ns.push_back(S); T.insert(T.end(), Tk, Tk + 12);
            slots.insert(slots.end(), s.begin(), s.end()); observes.insert(observes.end(), o.begin(), o.end()); px.insert(px.end(), x.begin(), x.end());
            level.insert(level.end(), l.begin(), l.end()); bearing.insert(bearing.end(), b.begin(), b.end());
        }
        return true;
    }
    DSDTM::TrackMapArrays arrays() const {
        DSDTM::TrackMapArrays m;
        m.sel.n_points = (int32_t)bad.size(); m.sel.p_world = p.data(); m.sel.bad = bad.data(); m.sel.n_keyframes = (int32_t)ns.size(); m.sel.T_kf_w = T.data();
        m.sel.n_slots = ns.data(); m.sel.slot_offset = off.data(); m.sel.point_of_slot = slots.data();
        m.found = found.data(); m.observes = observes.data(); m.px_xy = px.data(); m.level = level.data(); m.bearing = bearing.data();
        return m;
    }
    // the device map equals the mirror
    bool agrees() {
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
        CHECK(dsdtm_mapping_map_read(ctx, map, &im) == DSDTM_OK && im.complete == 1);
        CHECK(rp == p && rT == T && rbad == bad && rs == slots && ro == observes && rl == level && rb == bearing && rn == ns && roff == off);
        return true;
    }
    void close() { dsdtm_mapping_destroy(ctx); ctx = nullptr; }
};

// the caller's device arrays of a window call, and the host's index arrays
struct Arrays {
    dsdtm_mapping_window_arrays a{};
    std::vector<int32_t> h_kf, h_pt;
    std::vector<int64_t> h_slot;
    uint8_t* outlier = nullptr;
    int64_t nk, np, no;
    Arrays(int64_t kfs, int64_t pts, int64_t obs) : h_kf((size_t)kfs + 1), h_pt((size_t)pts + 1), h_slot((size_t)obs + 1), nk(kfs), np(pts), no(obs) {
        auto dev = [](size_t bytes) { void* q = nullptr; (void)hipMalloc(&q, bytes + 8); memset(q, 0xA5, bytes + 8); return q; };
        a.T_c2w = (double*)dev((size_t)kfs * 96); a.kf_constant = (uint8_t*)dev((size_t)kfs); a.points = (double*)dev((size_t)pts * 24);
        a.obs_kf = (int32_t*)dev((size_t)obs * 4); a.obs_point = (int32_t*)dev((size_t)obs * 4); a.obs_bearing = (double*)dev((size_t)obs * 24);
        a.obs_level = (int32_t*)dev((size_t)obs * 4); a.kf_index = (int32_t*)dev((size_t)kfs * 4); a.point_index = (int32_t*)dev((size_t)pts * 4);
        a.obs_slot = (int64_t*)dev((size_t)obs * 8); outlier = (uint8_t*)dev((size_t)obs);
        a.h_kf_index = h_kf.data(); a.h_point_index = h_pt.data(); a.h_obs_slot = h_slot.data();
        fill_a5(h_kf.data(), h_kf.size() * 4); fill_a5(h_pt.data(), h_pt.size() * 4); fill_a5(h_slot.data(), h_slot.size() * 8);
    }
    bool untouched() const {
        return all_a5(a.T_c2w, (size_t)nk * 96) && all_a5(a.points, (size_t)np * 24) && all_a5(a.obs_slot, (size_t)no * 8) && all_a5(a.kf_index, (size_t)nk * 4) &&
               all_a5(h_kf.data(), h_kf.size() * 4) && all_a5(h_pt.data(), h_pt.size() * 4) && all_a5(h_slot.data(), h_slot.size() * 8);
    }
    ~Arrays() {
        void* all[] = {a.T_c2w, a.kf_constant, a.points, a.obs_kf, a.obs_point, a.obs_bearing, a.obs_level, a.kf_index, a.point_index, a.obs_slot, outlier};
        for (void* q : all) (void)hipFree(q);
    }
};

// window -> (flags set by hand) -> commit for keyframe kf with cov, against the host functions on the mirror, which is updated
static bool chain(World& w, int kf, const std::vector<int32_t>& cov, int kcap, int pcap, int ocap, hipStream_t solver) {
    Arrays A(kcap, pcap, ocap);
    dsdtm_mapping_window_desc d = {w.map, kf, (int32_t)cov.size(), cov.data(), 0, kcap, pcap, ocap};
    dsdtm_local_ba_problem prob;
    dsdtm_mapping_window_result res;
    CHECK(dsdtm_mapping_ba_window(w.ctx, 1, &d, &A.a, &prob, &res) == DSDTM_OK);
    DSDTM::BaWindowHost h = DSDTM::ba_window_host(w.arrays(), kf, (int32_t)cov.size(), cov.data(), 0, kcap, pcap, ocap);
    CHECK(memcmp(&res, &h.result, sizeof res) == 0 && res.usable == 1 && prob.n_points == res.n_points && prob.keyframe_offset == 0);
    CHECK(memcmp(A.a.obs_slot, h.obs_slot.data(), h.obs_slot.size() * 8) == 0 && memcmp(A.h_slot.data(), h.obs_slot.data(), h.obs_slot.size() * 8) == 0);
    CHECK(memcmp(A.h_kf.data(), h.kf_index.data(), h.kf_index.size() * 4) == 0 && memcmp(A.a.T_c2w, h.T_c2w.data(), h.T_c2w.size() * 8) == 0);
    CHECK(all_a5(A.a.obs_slot + res.n_obs, (size_t)(ocap - res.n_obs) * 8 + 8) && all_a5(A.a.points + 3 * (size_t)res.n_points, (size_t)(pcap - res.n_points) * 24 + 8));
    std::vector<uint8_t> flags((size_t)res.n_obs);
    for (size_t j = 0; j < flags.size(); ++j) flags[j] = j % 3 == 0;
    memcpy(A.outlier, flags.data(), flags.size());
    for (int i = 0; i < res.n_points; ++i) A.a.points[3 * (size_t)i] += 0.5;       // in place of the solver
    std::vector<int32_t> bad_points(8);
    dsdtm_mapping_commit_result cr;
    CHECK(dsdtm_mapping_ba_commit(w.ctx, 1, &d, &prob, &res, &A.a, A.outlier, solver, 8, bad_points.data(), &cr) == DSDTM_OK);
    const DSDTM::MappingMapWritable wr = {w.p.data(), w.bad.data(), w.T.data(), w.off.data(), w.slots.data(), w.observes.data()};
    const DSDTM::BaCommitHost c = DSDTM::ba_commit_host(wr, h, A.a.T_c2w, A.a.points, flags.data());
    CHECK(cr.n_outliers == c.n_outliers && cr.n_bad == (int32_t)c.bad_points.size() && cr.n_outliers > 0 && cr.n_bad > 0);
    for (int i = 0; i < std::min(cr.n_bad, 8); ++i) CHECK(bad_points[(size_t)i] == c.bad_points[(size_t)i]);
    return w.agrees();
}

static bool windows_and_growth() {
    World w;
    CHECK(w.open(8, 24, 60, 7) && w.agrees());
    hipStream_t solver = nullptr;
    CHECK(hipStreamCreateWithFlags(&solver, hipStreamNonBlocking) == hipSuccess);
    std::vector<int32_t> k(32), wt(32);
    fill_a5(k.data(), 128); fill_a5(wt.data(), 128);
    dsdtm_mapping_cov_desc cd[2] = {{w.map, 3, 32, k.data(), wt.data()}, {w.map, 0, 0, nullptr, nullptr}};
    dsdtm_mapping_cov_result cr[2];
    CHECK(dsdtm_mapping_covisibility(w.ctx, 2, cd, cr) == DSDTM_OK);
    const DSDTM::CovisibilityHost c = DSDTM::update_connection_host(w.arrays(), 3);
    CHECK(cr[0].n_cov == (int32_t)c.cov_kf.size() && cr[0].n_cov > 0 && cr[0].n_connected == c.n_connected && memcmp(k.data(), c.cov_kf.data(), c.cov_kf.size() * 4) == 0);
    CHECK(all_a5(k.data() + cr[0].n_cov, (size_t)(32 - cr[0].n_cov) * 4) && cr[1].overflow == (cr[1].n_cov > 0));
    CHECK(chain(w, 3, {2, 4}, 16, 128, 512, solver));                      // small blocks first ...
    CHECK(chain(w, 6, {5, 7, 1}, 80, 4096, 131072, nullptr));
    {                                                                       // ... then both staging blocks must grow: four windows' pairs are 4 MB
        Arrays A(64, 512, 4 * (int64_t)DSDTM_LBA_MAX_OBSERVATIONS);
        const int32_t c0[1] = {0}, c5[1] = {5};
        dsdtm_mapping_window_desc d[4] = {{w.map, 1, 1, c0, -1, 16, 128, DSDTM_LBA_MAX_OBSERVATIONS}, {w.map, 6, 1, c5, -1, 16, 128, DSDTM_LBA_MAX_OBSERVATIONS},
                                          {w.map, 1, 1, c0, 1, 16, 128, DSDTM_LBA_MAX_OBSERVATIONS}, {w.map, 6, 1, c5, 5, 16, 128, DSDTM_LBA_MAX_OBSERVATIONS}};
        dsdtm_local_ba_problem prob[4];
        dsdtm_mapping_window_result res[4];
        const long d0 = fake_hip_calls("hipMalloc");
        CHECK(dsdtm_mapping_ba_window(w.ctx, 4, d, &A.a, prob, res) == DSDTM_OK && fake_hip_calls("hipMalloc") > d0);
        CHECK(res[0].usable && res[1].usable && res[2].usable && res[2].n_points == 0 && res[3].usable && prob[3].observation_offset == 3 * (int64_t)DSDTM_LBA_MAX_OBSERVATIONS);
        const DSDTM::BaWindowHost h = DSDTM::ba_window_host(w.arrays(), 6, 1, c5, -1, 16, 128, DSDTM_LBA_MAX_OBSERVATIONS);
        CHECK(memcmp(&res[1], &h.result, sizeof res[1]) == 0 && memcmp(A.a.obs_slot + DSDTM_LBA_MAX_OBSERVATIONS, h.obs_slot.data(), h.obs_slot.size() * 8) == 0);
        CHECK(memcmp(A.h_slot.data() + DSDTM_LBA_MAX_OBSERVATIONS, h.obs_slot.data(), h.obs_slot.size() * 8) == 0 && memcmp(A.h_pt.data() + 128, h.point_index.data(), h.point_index.size() * 4) == 0);
    }
    CHECK(chain(w, 1, {0}, 16, 128, 512, solver));
    CHECK(hipStreamDestroy(solver) == hipSuccess);
    w.close();
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_pending() == 0 && fake_hip_errors().empty());
    return true;
}

static bool validation() {
    World w;
    CHECK(w.open(6, 12, 30, 5));
    dsdtm_mapping_ctx* other = nullptr;
    dsdtm_trackmap* foreign = nullptr;
    CHECK(dsdtm_mapping_create(0, &other) == DSDTM_OK && dsdtm_mapping_map_create(other, &foreign) == DSDTM_OK);
    int32_t k[4], wt[4];
    dsdtm_mapping_cov_result cr;
    fill_a5(&cr, sizeof cr); fill_a5(k, sizeof k);
    auto cov = [&](dsdtm_mapping_cov_desc d, const char* needle) { return named_err(w.ctx, dsdtm_mapping_covisibility(w.ctx, 1, &d, &cr), needle) && all_a5(&cr, sizeof cr) && all_a5(k, sizeof k); };
    CHECK(cov({nullptr, 0, 4, k, wt}, "map is NULL") && cov({foreign, 0, 4, k, wt}, "not a map of this context") && cov({w.map, 6, 4, k, wt}, "kf is not"));
    CHECK(cov({w.map, 0, -1, k, wt}, "capacity") && cov({w.map, 0, 4, nullptr, wt}, "cov_kf is NULL") && cov({w.map, 0, 4, k, nullptr}, "cov_weight is NULL"));
    dsdtm_mapping_cov_desc good = {w.map, 0, 4, k, wt};
    CHECK(named_err(w.ctx, dsdtm_mapping_covisibility(w.ctx, -1, &good, &cr), "outside") && named_err(w.ctx, dsdtm_mapping_covisibility(w.ctx, 1025, &good, &cr), "outside"));
    CHECK(named_err(w.ctx, dsdtm_mapping_covisibility(w.ctx, 1, nullptr, &cr), "descs is NULL") && dsdtm_mapping_covisibility(w.ctx, 0, nullptr, nullptr) == DSDTM_OK);
    CHECK(dsdtm_mapping_covisibility(nullptr, 1, &good, &cr) == DSDTM_ERR_INVALID);
    // the window
    Arrays A(32, 256, 1024);
    const int32_t c1[2] = {1, 2}, twice[2] = {1, 1}, self[2] = {1, 0}, far[1] = {6};
    dsdtm_local_ba_problem prob[2];
    dsdtm_mapping_window_result res[2];
    fill_a5(prob, sizeof prob); fill_a5(res, sizeof res);
    auto win = [&](dsdtm_mapping_window_desc bad, const char* needle) {
        dsdtm_mapping_window_desc d[2] = {{w.map, 0, 2, c1, -1, 16, 128, 512}, bad};
        return named_err(w.ctx, dsdtm_mapping_ba_window(w.ctx, 2, d, &A.a, prob, res), needle) && strstr(dsdtm_mapping_last_error(w.ctx), "desc 1") && A.untouched() &&
               all_a5(prob, sizeof prob) && all_a5(res, sizeof res);
    };
    CHECK(win({nullptr, 0, 0, nullptr, -1, 16, 128, 512}, "map is NULL") && win({foreign, 0, 0, nullptr, -1, 16, 128, 512}, "not a map"));
    CHECK(win({w.map, -1, 0, nullptr, -1, 16, 128, 512}, "kf is not") && win({w.map, 0, 256, c1, -1, 16, 128, 512}, "n_cov") && win({w.map, 0, 2, nullptr, -1, 16, 128, 512}, "cov_kf is NULL"));
    CHECK(win({w.map, 0, 2, twice, -1, 16, 128, 512}, "repeats") && win({w.map, 0, 2, self, -1, 16, 128, 512}, "contains kf") && win({w.map, 0, 1, far, -1, 16, 128, 512}, "outside the map"));
    CHECK(win({w.map, 0, 2, c1, 6, 16, 128, 512}, "origin_kf") && win({w.map, 0, 2, c1, -1, -1, 128, 512}, "negative") && win({w.map, 0, 2, c1, -1, 16, 16385, 512}, "point_capacity"));
    CHECK(win({w.map, 0, 2, c1, -1, 16, 128, 131073}, "observation_capacity"));
    dsdtm_mapping_window_desc d[2] = {{w.map, 0, 2, c1, -1, 16, 128, 512}, {w.map, 4, 1, c1 + 1, -1, 16, 128, 512}};
    dsdtm_mapping_window_arrays hole = A.a;
    hole.obs_level = nullptr;
    CHECK(named_err(w.ctx, dsdtm_mapping_ba_window(w.ctx, 2, d, &hole, prob, res), "obs_level is NULL") && named_err(w.ctx, dsdtm_mapping_ba_window(w.ctx, 257, d, &A.a, prob, res), "outside"));
    CHECK(named_err(w.ctx, dsdtm_mapping_ba_window(w.ctx, 2, d, &A.a, nullptr, res), "problems is NULL") && A.untouched());
    CHECK(dsdtm_mapping_ba_window(w.ctx, 2, d, &A.a, prob, res) == DSDTM_OK && res[0].usable && res[1].usable && prob[1].point_offset == 128);
    // the commit: nothing of the map is written by a refused call
    int32_t bad_points[8];
    dsdtm_mapping_commit_result out[2];
    memset(A.outlier, 0, 1024);
    auto commit = [&](const dsdtm_mapping_window_desc* dd, const dsdtm_local_ba_problem* pp, const dsdtm_mapping_window_arrays* aa, int cap, const char* needle) {
        return named_err(w.ctx, dsdtm_mapping_ba_commit(w.ctx, 2, dd, pp, res, aa, A.outlier, nullptr, cap, bad_points, out), needle) && w.agrees();
    };
    CHECK(commit(d, prob, &A.a, -1, "bad_capacity") && commit(d, prob, &A.a, 16385, "bad_capacity") && commit(nullptr, prob, &A.a, 8, "descs is NULL"));
    CHECK(commit(d, nullptr, &A.a, 8, "problems is NULL") && commit(d, prob, nullptr, 8, "arrays is NULL") && commit(d, prob, &hole, 8, "obs_level is NULL"));
    dsdtm_local_ba_problem moved[2] = {prob[0], prob[1]};
    moved[1].observation_offset += 1;
    CHECK(commit(d, moved, &A.a, 8, "desc 1: problems: the offsets"));
    moved[1] = prob[1]; moved[0].n_keyframes = 17;
    CHECK(commit(d, moved, &A.a, 8, "desc 0: problems: a count exceeds"));
    CHECK(named_err(w.ctx, dsdtm_mapping_ba_commit(w.ctx, 2, d, prob, res, &A.a, nullptr, nullptr, 8, bad_points, out), "outlier is NULL"));
    CHECK(named_err(w.ctx, dsdtm_mapping_ba_commit(w.ctx, 2, d, prob, res, &A.a, A.outlier, nullptr, 8, nullptr, out), "bad_points is NULL"));
    const bool share = res[0].n_fixed + res[1].n_fixed > 0;                 // (keyframes 0-2 and 4, 2: they share keyframe 2)
    CHECK(share && commit(d, prob, &A.a, 8, "windows 0 and 1 share"));
    res[1].usable = 0;                                                      // a window that is not usable is skipped: no overlap left
    fill_a5(out, sizeof out);
    CHECK(dsdtm_mapping_ba_commit(w.ctx, 2, d, prob, res, &A.a, A.outlier, nullptr, 0, nullptr, out) == DSDTM_OK && out[0].n_outliers == 0 && out[1].n_bad == 0 && out[1].reserved == 0);
    dsdtm_mapping_destroy(other);
    w.close();
    CHECK(fake_hip_errors().empty());
    return true;
}

// every HIP call and every launch on the way of the three entries failing once: DSDTM_ERR_HIP, nothing leaks (the commit's event), the
// context stays usable, and a failed commit that got no further than its check has written nothing
static bool hip_failures() {
    for (int entry = 0; entry < 3; ++entry)
        for (const char* api : {"hipMemcpyAsync", "hipStreamSynchronize", "hipMalloc", "hipHostMalloc", "hipSetDevice", "hipEventCreateWithFlags", "hipEventRecord",
                                "hipStreamWaitEvent", "launch"})
            for (long nth = 1; nth <= 4; ++nth) {
                World w;
                CHECK(w.open(6, 12, 30, 5));
                const bool launch = strcmp(api, "launch") == 0;
                Arrays A(16, 128, 512);
                const int32_t c1[2] = {1, 2};
                dsdtm_mapping_window_desc d = {w.map, 0, 2, c1, -1, 16, 128, 512};
                dsdtm_local_ba_problem prob;
                dsdtm_mapping_window_result res;
                int32_t k[8], wt[8], bad_points[8];
                dsdtm_mapping_cov_desc cd = {w.map, 0, 8, k, wt};
                dsdtm_mapping_cov_result cr;
                dsdtm_mapping_commit_result out;
                if (entry == 2) { CHECK(dsdtm_mapping_ba_window(w.ctx, 1, &d, &A.a, &prob, &res) == DSDTM_OK && res.usable); memset(A.outlier, 1, 512); }
                fill_a5(&cr, sizeof cr); fill_a5(&out, sizeof out);
                if (entry != 2) { fill_a5(&prob, sizeof prob); fill_a5(&res, sizeof res); }
                if (launch) fake_mapping_fail(nth); else fake_hip_fail(api, nth);
                int rc;
                if (entry == 0) rc = dsdtm_mapping_covisibility(w.ctx, 1, &cd, &cr);
                else if (entry == 1) rc = dsdtm_mapping_ba_window(w.ctx, 1, &d, &A.a, &prob, &res);
                else rc = dsdtm_mapping_ba_commit(w.ctx, 1, &d, &prob, &res, &A.a, A.outlier, nullptr, 8, bad_points, &out);
                fake_mapping_fail(0);
                if (!launch) fake_hip_fail(api, 0);
                if (rc != DSDTM_OK) {
                    CHECK(rc == DSDTM_ERR_HIP && strlen(dsdtm_mapping_last_error(w.ctx)) > 0);
                    if (entry == 0) CHECK(all_a5(&cr, sizeof cr));
                    if (entry == 1) CHECK(all_a5(&prob, sizeof prob) && all_a5(&res, sizeof res));
                }
                // the context is usable whatever happened; the first two entries never write the map
                CHECK(dsdtm_mapping_covisibility(w.ctx, 1, &cd, &cr) == DSDTM_OK && dsdtm_mapping_ba_window(w.ctx, 1, &d, &A.a, &prob, &res) == DSDTM_OK);
                if (entry != 2) CHECK(w.agrees() && res.usable && dsdtm_mapping_ba_commit(w.ctx, 1, &d, &prob, &res, &A.a, A.outlier, nullptr, 8, bad_points, &out) == DSDTM_OK);
                w.close();
                CHECK(fake_hip_pending() == 0);
            }
    CHECK(fake_hip_live_allocations() == 0 && fake_hip_errors().empty());
    return true;
}

// the limits at their values, and the call whose block would exceed DSDTM_TRACKMAP_MAX_CALL_BYTES
static bool limits() {
    World w;
    CHECK(w.open(64, 1024, 4096, 512));
    std::vector<int32_t> cov;
    for (int k = 0; k < 63; ++k) cov.push_back(k);
    const int n = DSDTM_MAPPING_MAX_WINDOWS;
    std::vector<dsdtm_mapping_window_desc> d((size_t)n, dsdtm_mapping_window_desc{w.map, 63, 63, cov.data(), -1, 0, 0, 0});
    std::vector<dsdtm_local_ba_problem> prob((size_t)n);
    std::vector<dsdtm_mapping_window_result> res((size_t)n);
    dsdtm_mapping_window_arrays none{};
    // 256 windows of 64 keyframes with no room at all: counted in full, none usable, nothing written
    CHECK(dsdtm_mapping_ba_window(w.ctx, n, d.data(), &none, prob.data(), res.data()) == DSDTM_OK);
    for (int t = 0; t < n; ++t)
        CHECK(res[(size_t)t].n_local == 64 && res[(size_t)t].over_free_kf && res[(size_t)t].over_keyframe_capacity && res[(size_t)t].over_point_capacity && !res[(size_t)t].usable &&
              res[(size_t)t].n_points == res[0].n_points && res[0].n_points > 0 && prob[(size_t)t].n_keyframes == 0);
    // 256 windows over 256 keyframes of 4096 slots each: 1 M entries per window, 36 MB of table and counters each — refused, nothing enqueued
    fill_a5(res.data(), res.size() * sizeof res[0]);
    World huge;
    CHECK(huge.open(256, DSDTM_LOCALMAP_MAX_SLOTS, 64, 1));
    std::vector<int32_t> all;
    for (int k = 0; k < 255; ++k) all.push_back(k);
    std::vector<dsdtm_mapping_window_desc> dh((size_t)n, dsdtm_mapping_window_desc{huge.map, 255, 255, all.data(), -1, 0, 0, 0});
    CHECK(named_err(huge.ctx, dsdtm_mapping_ba_window(huge.ctx, n, dh.data(), &none, prob.data(), res.data()), "exceeds") && all_a5(res.data(), res.size() * sizeof res[0]));
    CHECK(dsdtm_mapping_ba_window(huge.ctx, 1, dh.data(), &none, prob.data(), res.data()) == DSDTM_OK && res[0].n_local == 256 && !res[0].usable);
    huge.close();
    w.close();
    CHECK(fake_hip_errors().empty());
    return true;
}

static bool create_failures() {
    return addon_create_failures("dsdtm_amd_mapping", dsdtm_mapping_create, dsdtm_mapping_destroy, dsdtm_mapping_last_error);
}

int main(int argc, char** argv) {
    const std::pair<std::string, bool (*)()> all[] = {{"windows_and_growth", windows_and_growth}, {"validation", validation}, {"hip_failures", hip_failures},
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
