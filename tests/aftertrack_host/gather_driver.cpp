// gather_keyframe_desc_host (dsdtm_amd/host/dsdtm_slam_host.hpp: plain C++, no device call, no library) on the trackers
// tests/test_aftertrack_cpu.py writes; the gathered lists go back as a flat binary file that the test holds against the restatement,
// bit for bit. Build: g++ -O2 -std=c++14 -ffp-contract=off. Usage: gather_driver <cases.bin> <answers.bin>
#include <cstdio>
#include <cstdlib>

#include "../../dsdtm_amd/host/dsdtm_slam_host.hpp"

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

int main(int argc, char** argv) {
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 1;
    const int32_t n_jobs = take<int32_t>(1)[0];
    for (int32_t job = 0; job < n_jobs; ++job) {
        const std::vector<int32_t> head = take<int32_t>(2);
        const size_t P = (size_t)head[0], K = (size_t)head[1];
        const std::vector<double> p_world = take<double>(3 * P);
        const std::vector<uint8_t> bad = take<uint8_t>(P);
        const std::vector<double> T = take<double>(12 * K);
        const std::vector<int32_t> n_slots = take<int32_t>(K);
        std::vector<int64_t> off(K);
        size_t S = 0;
        for (size_t k = 0; k < K; ++k) { off[k] = (int64_t)S; S += (size_t)n_slots[k]; }
        const std::vector<int32_t> slots = take<int32_t>(S);
        DSDTM::TrackMapArrays t;
        t.sel.n_points = (int32_t)P; t.sel.p_world = p_world.data(); t.sel.bad = bad.data();
        t.sel.n_keyframes = (int32_t)K; t.sel.T_kf_w = T.data(); t.sel.n_slots = n_slots.data(); t.sel.slot_offset = off.data(); t.sel.point_of_slot = slots.data();
        const std::vector<double> T_cur = take<double>(12);
        const std::vector<int32_t> q = take<int32_t>(4);                    // n_valid, n_cur, kf, n_lkf
        const std::vector<int32_t> cur = take<int32_t>((size_t)q[1]), lk = take<int32_t>((size_t)q[3]);
        const DSDTM::KeyframeDescHost h = DSDTM::gather_keyframe_desc_host(t, T_cur.data(), q[0], q[1], cur.data(), q[2], q[3], lk.data());
        const int32_t counts[4] = {h.n_valid, (int32_t)h.cur_bad.size(), (int32_t)h.kf_bad.size(), (int32_t)(h.local_kf_centre.size() / 3)};
        fwrite(counts, 4, 4, out);
        fwrite(h.T_cur_w, 8, 12, out); fwrite(h.T_kf_w, 8, 12, out);
        put(h.cur_p_world); put(h.cur_bad); put(h.kf_p_world); put(h.kf_bad); put(h.local_kf_centre);
    }
    fclose(out);
    return 0;
}
