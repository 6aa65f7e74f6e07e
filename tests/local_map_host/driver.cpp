// select_local_map_host (dsdtm_amd/host/dsdtm_localmap_host.hpp) on the cases tests/test_local_map_cpu.py writes: no device, no library.
// Input (binary, native endianness): int32 n_cases; per case int32 n_local, boundary, capacity, P, K, n_poses; P x 3 doubles; P bytes;
// K x 12 doubles; K int32 slot counts; the slots; n_poses x 12 doubles. Output: one line per case and pose — the four counters, then
// the lists, distances as their 64-bit patterns in hex. With `time REPS` behind the file name (tools/time_local_map.py) each case is
// walked REPS times over all its poses first, on one thread with a scratch kept between calls, and a line `time <case> <median> <p10>
// <p90>` gives the microseconds per select. Test infrastructure only.
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../dsdtm_amd/host/dsdtm_localmap_host.hpp"

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const dsdtm_camera cam{512.f, 512.f, 320.f, 240.f, 512.f, 640, 480};
    const int time_reps = argc >= 4 && std::string(argv[2]) == "time" ? std::atoi(argv[3]) : 0;
    const int n_cases = take<int32_t>(f, 1)[0];
    DSDTM::LocalMapHostScratch scratch;
    for (int c = 0; c < n_cases; ++c) {
        const std::vector<int32_t> hd = take<int32_t>(f, 6);
        const int n_local = hd[0], boundary = hd[1], capacity = hd[2], P = hd[3], K = hd[4], n_poses = hd[5];
        const std::vector<double> p = take<double>(f, 3 * (size_t)P);
        const std::vector<uint8_t> bad = take<uint8_t>(f, (size_t)P);
        const std::vector<double> T = take<double>(f, 12 * (size_t)K);
        const std::vector<int32_t> ns = take<int32_t>(f, (size_t)K);
        std::vector<int64_t> off((size_t)K);
        int64_t total = 0;
        for (int k = 0; k < K; ++k) { off[(size_t)k] = total; total += ns[(size_t)k]; }
        const std::vector<int32_t> slots = take<int32_t>(f, (size_t)total);
        const std::vector<double> poses = take<double>(f, 12 * (size_t)n_poses);
        DSDTM::LocalMapArrays m;
        m.n_points = P; m.p_world = p.data(); m.bad = bad.data(); m.n_keyframes = K; m.T_kf_w = T.data(); m.n_slots = ns.data();
        m.slot_offset = off.data(); m.point_of_slot = slots.data();
        const dsdtm_localmap_params prm{n_local, boundary};
        if (time_reps > 0) {
            std::vector<int32_t> kf((size_t)n_local), point((size_t)capacity + 1), point_kf((size_t)capacity + 1);
            std::vector<double> dist((size_t)n_local), us;
            dsdtm_localmap_result r;
            for (int rep = -1; rep < time_reps; ++rep) {          // (the first walk is the warm-up)
                const auto t0 = std::chrono::steady_clock::now();
                for (int q = 0; q < n_poses; ++q)
                    DSDTM::select_local_map_host(cam, prm, m, poses.data() + 12 * (size_t)q, kf.data(), dist.data(), capacity, point.data(), point_kf.data(), &r, &scratch);
                const double t = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / (n_poses > 0 ? n_poses : 1);
                if (rep >= 0) us.push_back(t);
            }
            std::sort(us.begin(), us.end());
            std::printf("time %d %.3f %.3f %.3f\n", c, us[us.size() / 2], us[us.size() / 10], us[(9 * us.size()) / 10]);
        }
        for (int q = 0; q < n_poses; ++q) {
            std::vector<int32_t> kf((size_t)n_local, -7), point((size_t)capacity + 1, -7), point_kf((size_t)capacity + 1, -7);
            std::vector<double> dist((size_t)n_local, -7.0);
            dsdtm_localmap_result r;
            DSDTM::select_local_map_host(cam, prm, m, poses.data() + 12 * (size_t)q, kf.data(), dist.data(), capacity, point.data(), point_kf.data(), &r,
                                         q % 2 ? &scratch : nullptr);
            if (point[(size_t)capacity] != -7 || point_kf[(size_t)capacity] != -7) { std::fprintf(stderr, "written past the capacity\n"); return 3; }
            std::printf("%d %d %d %d %d %d |", c, q, r.n_close, r.n_kf, r.n_points, r.overflow);
            for (int i = 0; i < r.n_kf; ++i) std::printf(" %d", kf[(size_t)i]);
            std::printf(" |");
            for (int i = 0; i < r.n_kf; ++i) { uint64_t b; std::memcpy(&b, &dist[(size_t)i], 8); std::printf(" %016" PRIx64, b); }
            const int np = r.n_points < capacity ? r.n_points : capacity;
            std::printf(" |");
            for (int i = 0; i < np; ++i) std::printf(" %d", point[(size_t)i]);
            std::printf(" |");
            for (int i = 0; i < np; ++i) std::printf(" %d", point_kf[(size_t)i]);
            std::printf("\n");
        }
    }
    std::fclose(f);
    return 0;
}
