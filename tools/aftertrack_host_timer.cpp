// Times track_commit_host and gather_keyframe_desc_host (dsdtm_amd/host/dsdtm_slam_host.hpp) on one thread over a world that
// tools/time_aftertrack.py writes. Build: g++ -O2 -std=c++14 -ffp-contract=off. Usage: aftertrack_host_timer <world.bin>
// Prints `<name> <median us> <p10> <p90>` per row.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../dsdtm_amd/host/dsdtm_slam_host.hpp"

static FILE* in;
template <class T>
static std::vector<T> take(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
static void report(const char* name, std::vector<double>& us) {
    std::sort(us.begin(), us.end());
    printf("%s %.3f %.3f %.3f\n", name, us[us.size() / 2], us[us.size() / 10], us[9 * us.size() / 10]);
}

int main(int argc, char** argv) {
    if (argc != 2 || !(in = fopen(argv[1], "rb"))) return 1;
    const std::vector<int32_t> head = take<int32_t>(2);
    const size_t P = (size_t)head[0], K = (size_t)head[1];
    const std::vector<double> p_world = take<double>(3 * P);
    std::vector<uint8_t> bad = take<uint8_t>(P);
    std::vector<int32_t> found = take<int32_t>(P);
    const std::vector<double> T = take<double>(12 * K);
    const std::vector<int32_t> n_slots = take<int32_t>(K);
    std::vector<int64_t> off(K);
    size_t S = 0;
    for (size_t k = 0; k < K; ++k) { off[k] = (int64_t)S; S += (size_t)n_slots[k]; }
    std::vector<int32_t> slots = take<int32_t>(S);
    std::vector<uint8_t> observes = take<uint8_t>(S);
    const std::vector<int32_t> q = take<int32_t>(5);                        // n_matches, reps, n_cur, kf, n_lkf
    const std::vector<int32_t> match = take<int32_t>((size_t)q[0]), victims = take<int32_t>((size_t)q[1]);
    const std::vector<int32_t> cur = take<int32_t>((size_t)q[2]), lk = take<int32_t>((size_t)q[4]);
    const int reps = q[1];
    DSDTM::TrackCommitMap m;
    m.n_points = (int32_t)P; m.found = found.data(); m.bad = bad.data(); m.n_slots_total = (int64_t)S; m.point_of_slot = slots.data(); m.observes = observes.data();
    std::vector<double> norm((size_t)q[0], 0.0), us;
    auto now = [] { return std::chrono::steady_clock::now(); };
    for (int r = 0; r < reps; ++r) {                                        // no erase: the matches alone
        const auto t0 = now();
        const DSDTM::TrackCommitHost h = DSDTM::track_commit_host(m, 1.0, q[0], match.data(), norm.data());
        us.push_back(std::chrono::duration<double, std::micro>(now() - t0).count() + 0.0 * h.n_erased);
    }
    report("track_commit_host_no_bad", us);
    us.clear();
    for (int r = 0; r < reps; ++r) {                                        // one point goes bad: the pass over the slots
        std::vector<int32_t> pts = match;
        std::vector<double> nr = norm;
        pts[0] = victims[(size_t)r]; nr[0] = 2.0;
        found[(size_t)pts[0]] = 0;
        const auto t0 = now();
        const DSDTM::TrackCommitHost h = DSDTM::track_commit_host(m, 1.0, q[0], pts.data(), nr.data());
        us.push_back(std::chrono::duration<double, std::micro>(now() - t0).count() + 0.0 * h.n_erased);
    }
    report("track_commit_host_one_bad", us);
    us.clear();
    DSDTM::TrackMapArrays t;
    t.sel.n_points = (int32_t)P; t.sel.p_world = p_world.data(); t.sel.bad = bad.data(); t.sel.n_keyframes = (int32_t)K; t.sel.T_kf_w = T.data(); t.sel.n_slots = n_slots.data();
    t.sel.slot_offset = off.data(); t.sel.point_of_slot = slots.data();
    double sink = 0;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = now();
        const DSDTM::KeyframeDescHost h = DSDTM::gather_keyframe_desc_host(t, T.data(), q[2], q[2], cur.data(), q[3], q[4], lk.data());
        us.push_back(std::chrono::duration<double, std::micro>(now() - t0).count());
        sink += h.kf_p_world.empty() ? 0.0 : h.kf_p_world[0];
    }
    report("gather_keyframe_desc_host", us);
    return sink == 12345.678 ? 3 : 0;
}
