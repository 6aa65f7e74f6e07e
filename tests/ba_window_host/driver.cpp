// update_connection_host, ba_window_host and ba_commit_host (dsdtm_amd/host/dsdtm_mapping_host.hpp: plain C++, no device call, no
// library) on the cases tests/test_ba_window_cpu.py writes; the answers go back as a flat binary file that the test holds against the
// restatement, integers equal and doubles bit-equal. Build: g++ -O2 -std=c++14 -ffp-contract=off. Usage: driver <cases.bin> <answers.bin>
#include <cstdio>
#include <cstdlib>

#include "../../dsdtm_amd/host/dsdtm_mapping_host.hpp"

static FILE* in;
static FILE* out;

template <class T>
static std::vector<T> take(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, in) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
template <class T>
static void put(const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), out); }
static void put_int(int32_t v) { fwrite(&v, 4, 1, out); }

int main(int argc, char** argv) {
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 1;
    const int32_t n_jobs = take<int32_t>(1)[0];
    for (int32_t job = 0; job < n_jobs; ++job) {
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
        DSDTM::TrackMapArrays t;
        t.sel.n_points = (int32_t)P; t.sel.p_world = p_world.data(); t.sel.bad = bad.data();
        t.sel.n_keyframes = (int32_t)K; t.sel.T_kf_w = T.data(); t.sel.n_slots = n_slots.data(); t.sel.slot_offset = off.data();
        t.sel.point_of_slot = slots.data();
        t.found = found.data(); t.observes = observes.data(); t.px_xy = px.data(); t.level = level.data(); t.bearing = bearing.data();
        const int32_t n_cov_requests = take<int32_t>(1)[0];
        for (int32_t q = 0; q < n_cov_requests; ++q) {
            const DSDTM::CovisibilityHost c = DSDTM::update_connection_host(t, take<int32_t>(1)[0]);
            put_int(c.n_connected); put_int((int32_t)c.cov_kf.size());
            put(c.cov_kf); put(c.cov_weight);
        }
        const int32_t n_windows = take<int32_t>(1)[0];
        for (int32_t q = 0; q < n_windows; ++q) {
            const std::vector<int32_t> w = take<int32_t>(2);            // kf, n_cov
            const std::vector<int32_t> cov = take<int32_t>((size_t)w[1]);
            const std::vector<int32_t> rest = take<int32_t>(5);         // origin, the three capacities, commit (0 / 1)
            DSDTM::BaWindowHost win = DSDTM::ba_window_host(t, w[0], w[1], cov.data(), rest[0], rest[1], rest[2], rest[3]);
            fwrite(&win.result, sizeof win.result, 1, out);
            if (!win.result.usable) continue;
            put(win.kf_index); put(win.kf_constant); put(win.T_c2w); put(win.point_index); put(win.points);
            put(win.obs_kf); put(win.obs_point); put(win.obs_slot); put(win.obs_bearing); put(win.obs_level);
            if (!rest[4]) continue;
            const std::vector<uint8_t> outlier = take<uint8_t>(win.obs_point.size());
            for (size_t i = 0; i < win.kf_index.size(); ++i) win.T_c2w[12 * i + 3] += 0.25;      // in place of the solver (the test does the same)
            for (double& v : win.points) v += 0.125;
            const DSDTM::MappingMapWritable m = {p_world.data(), bad.data(), T.data(), off.data(), slots.data(), observes.data()};
            const DSDTM::BaCommitHost c = DSDTM::ba_commit_host(m, win, win.T_c2w.data(), win.points.data(), outlier.data());
            put_int(c.n_outliers); put_int((int32_t)c.bad_points.size());
            put(c.bad_points);
        }
        put(p_world); put(bad); put(T); put(slots); put(observes);      // the map after the commits
    }
    fclose(out);
    return 0;
}
