// Times update_connection_host, ba_window_host and ba_commit_host (dsdtm_amd/host/dsdtm_mapping_host.hpp) on one thread for
// tools/time_ba_window.py. Input: one world in the format of tests/ba_window_host/driver.cpp, then kf, origin_kf, n_cov, cov_kf, reps.
// Prints "name median_us p10_us p90_us" per function and the window's counts. The commit runs on a fresh copy of the map each time
// (the copy is outside the clock), with no observation flagged, as the device commit of the tool is timed. Build: g++ -O2 -std=c++14 -ffp-contract=off.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../dsdtm_amd/host/dsdtm_mapping_host.hpp"

static FILE* in;
template <class T>
static std::vector<T> take(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static void report(const char* name, std::vector<double>& t) {
    std::sort(t.begin(), t.end());
    printf("%s %.2f %.2f %.2f\n", name, t[t.size() / 2], t[t.size() / 10], t[(9 * t.size()) / 10]);
}

int main(int argc, char** argv) {
    if (argc != 2 || !(in = fopen(argv[1], "rb"))) return 1;
    const std::vector<int32_t> head = take<int32_t>(2);
    const size_t P = (size_t)head[0], K = (size_t)head[1];
    std::vector<double> p_world = take<double>(3 * P);
    std::vector<uint8_t> bad = take<uint8_t>(P);
    std::vector<int32_t> found = take<int32_t>(P);
    std::vector<double> T = take<double>(12 * K);
    std::vector<int32_t> n_slots = take<int32_t>(K);
    std::vector<int64_t> off(K);
    size_t S = 0;
    for (size_t k = 0; k < K; ++k) { off[k] = (int64_t)S; S += (size_t)n_slots[k]; }
    std::vector<int32_t> slots = take<int32_t>(S);
    std::vector<uint8_t> observes = take<uint8_t>(S);
    std::vector<float> px = take<float>(2 * S);
    std::vector<int32_t> level = take<int32_t>(S);
    std::vector<double> bearing = take<double>(3 * S);
    const std::vector<int32_t> q = take<int32_t>(3);      // kf, origin, n_cov
    const std::vector<int32_t> cov = take<int32_t>((size_t)q[2]);
    const int reps = take<int32_t>(1)[0];
    DSDTM::TrackMapArrays t;
    t.sel.n_points = (int32_t)P; t.sel.p_world = p_world.data(); t.sel.bad = bad.data(); t.sel.n_keyframes = (int32_t)K; t.sel.T_kf_w = T.data();
    t.sel.n_slots = n_slots.data(); t.sel.slot_offset = off.data(); t.sel.point_of_slot = slots.data();
    t.found = found.data(); t.observes = observes.data(); t.px_xy = px.data(); t.level = level.data(); t.bearing = bearing.data();
    std::vector<double> tc, tw, tm;
    size_t sink = 0;
    DSDTM::BaWindowHost w;
    for (int r = 0; r < reps + 2; ++r) {
        double t0 = now_us();
        const DSDTM::CovisibilityHost c = DSDTM::update_connection_host(t, q[0]);
        double t1 = now_us();
        w = DSDTM::ba_window_host(t, q[0], q[2], cov.data(), q[1], 80, DSDTM_LBA_MAX_POINTS, DSDTM_LBA_MAX_OBSERVATIONS);
        double t2 = now_us();
        sink += c.cov_kf.size() + w.obs_kf.size();
        if (r >= 2) { tc.push_back(t1 - t0); tw.push_back(t2 - t1); }
        if (!w.result.usable) continue;
        std::vector<double> p2 = p_world, T2 = T;
        std::vector<uint8_t> bad2 = bad, obs2 = observes, flags(w.obs_point.size());
        std::vector<int32_t> slots2 = slots;
        const DSDTM::MappingMapWritable m = {p2.data(), bad2.data(), T2.data(), off.data(), slots2.data(), obs2.data()};
        t0 = now_us();
        const DSDTM::BaCommitHost cm = DSDTM::ba_commit_host(m, w, w.T_c2w.data(), w.points.data(), flags.data());
        t1 = now_us();
        sink += cm.bad_points.size();
        if (r >= 2) tm.push_back(t1 - t0);
    }
    report("update_connection_host", tc);
    report("ba_window_host", tw);
    if (!tm.empty()) report("ba_commit_host", tm);
    printf("window %d %d %d %d %d %zu\n", w.result.n_local, w.result.n_fixed, w.result.n_points, w.result.n_obs, w.result.usable, sink);
    return 0;
}
