// Runs select_local_map_host + flatten_local_map_host (dsdtm_amd/host/dsdtm_trackmap_host.hpp) on the cases tests/track_map_cases.py
// wrote and writes every answer, raw, for tests/test_track_map_cpu.py to hold against the restatement. Test infrastructure only.
//   driver <cases.bin> <answers.bin> [reps]      (reps: also prints `time <case> <median> <p10> <p90> <select median>` in us per pose)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dsdtm_amd/host/dsdtm_trackmap_host.hpp"

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
template <class T>
static void put(FILE* f, const T* p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "short write\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) return 2;
    const int reps = argc == 4 ? atoi(argv[3]) : 0;
    std::vector<double> sel_us;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const dsdtm_camera cam{512.f, 512.f, 320.f, 240.f, 512.f, 640, 480};
    const int n_cases = take<int32_t>(in, 1)[0];
    DSDTM::LocalMapHostScratch sel_scratch;
    for (int c = 0; c < n_cases; ++c) {
        const std::vector<int32_t> head = take<int32_t>(in, 6);
        const int n_local = head[0], cap = head[1], ocap = head[2], P = head[3], K = head[4], n_poses = head[5];
        const std::vector<double> p = take<double>(in, 3 * (size_t)P);
        const std::vector<uint8_t> bad = take<uint8_t>(in, (size_t)P);
        const std::vector<int32_t> found = take<int32_t>(in, (size_t)P);
        const std::vector<double> T = take<double>(in, 12 * (size_t)K);
        const std::vector<int32_t> ns = take<int32_t>(in, (size_t)K);
        std::vector<int64_t> off((size_t)K);
        size_t S = 0;
        for (int k = 0; k < K; ++k) { off[(size_t)k] = (int64_t)S; S += (size_t)ns[(size_t)k]; }
        const std::vector<int32_t> slots = take<int32_t>(in, S);
        const std::vector<uint8_t> observes = take<uint8_t>(in, S);
        const std::vector<float> px = take<float>(in, 2 * S);
        const std::vector<int32_t> level = take<int32_t>(in, S);
        const std::vector<double> bearing = take<double>(in, 3 * S);
        const std::vector<double> poses = take<double>(in, 12 * (size_t)n_poses);
        DSDTM::TrackMapArrays m;
        m.sel.n_points = P; m.sel.p_world = p.data(); m.sel.bad = bad.data(); m.sel.n_keyframes = K; m.sel.T_kf_w = T.data(); m.sel.n_slots = ns.data();
        m.sel.slot_offset = off.data(); m.sel.point_of_slot = slots.data();
        m.found = found.data(); m.observes = observes.data(); m.px_xy = px.data(); m.level = level.data(); m.bearing = bearing.data();
        DSDTM::TrackMapHostScratch scratch;      // (kept across the poses of a case: the second call meets a used one)
        if (reps > 0) {                          // tools/time_track_map.py: the host baseline, one thread, scratch and outputs kept between calls
            const size_t C = (size_t)cap + 1, O = (size_t)ocap + 1;
            std::vector<int32_t> kf((size_t)n_local), point(C), point_kf(C), mf(C), oo(C + 1), okf(O), olv(O);
            std::vector<double> kd((size_t)n_local), pw(3 * C), ob(3 * O), us;
            std::vector<uint8_t> mb(C);
            std::vector<float> opx(2 * O);
            for (int rep = -1; rep < reps; ++rep)
                for (int q = 0; q < n_poses; ++q) {
                    dsdtm_localmap_result r;
                    int32_t n_obs = 0;
                    const auto t0 = std::chrono::steady_clock::now();
                    DSDTM::select_local_map_host(cam, dsdtm_localmap_params{n_local, 0}, m.sel, &poses[12 * (size_t)q], kf.data(), kd.data(), cap, point.data(),
                                                 point_kf.data(), &r, &sel_scratch);
                    const auto t1 = std::chrono::steady_clock::now();
                    DSDTM::flatten_local_map_host(m, r.n_points < cap ? r.n_points : cap, point.data(), ocap, pw.data(), mf.data(), mb.data(), oo.data(),
                                                  okf.data(), opx.data(), olv.data(), ob.data(), &n_obs, &scratch);
                    const auto t2 = std::chrono::steady_clock::now();
                    if (rep >= 0) { us.push_back(std::chrono::duration<double, std::micro>(t2 - t0).count()); sel_us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count()); }
                }
            std::sort(us.begin(), us.end());
            std::sort(sel_us.begin(), sel_us.end());
            printf("time %d %.2f %.2f %.2f %.2f\n", c, us[us.size() / 2], us[us.size() / 10], us[9 * us.size() / 10], sel_us[sel_us.size() / 2]);
            sel_us.clear();
        }
        for (int q = 0; q < n_poses; ++q) {
            const size_t C = (size_t)cap + 1, O = (size_t)ocap + 1;
            std::vector<int32_t> kf((size_t)n_local), point(C), point_kf(C), mf(C), oo(C + 1), okf(O), olv(O);
            std::vector<double> kd((size_t)n_local), pw(3 * C), ob(3 * O);
            std::vector<uint8_t> mb(C);
            std::vector<float> opx(2 * O);
            dsdtm_localmap_result r;
            int32_t n_obs = 0;
            DSDTM::select_local_map_host(cam, dsdtm_localmap_params{n_local, 0}, m.sel, &poses[12 * (size_t)q], kf.data(), kd.data(), cap, point.data(),
                                         point_kf.data(), &r, &sel_scratch);
            const int32_t em = r.n_points < cap ? r.n_points : cap;
            DSDTM::flatten_local_map_host(m, em, point.data(), ocap, pw.data(), mf.data(), mb.data(), oo.data(), okf.data(), opx.data(), olv.data(),
                                          ob.data(), &n_obs, &scratch);
            const int32_t no = n_obs < ocap ? n_obs : ocap;
            const int32_t h[6] = {r.n_close, r.n_kf, r.n_points, n_obs, em, no};
            put(out, h, 6);
            put(out, kf.data(), (size_t)r.n_kf); put(out, kd.data(), (size_t)r.n_kf);
            put(out, point.data(), (size_t)em); put(out, point_kf.data(), (size_t)em);
            put(out, pw.data(), 3 * (size_t)em); put(out, mf.data(), (size_t)em); put(out, mb.data(), (size_t)em); put(out, oo.data(), (size_t)em + 1);
            put(out, okf.data(), (size_t)no); put(out, opx.data(), 2 * (size_t)no); put(out, olv.data(), (size_t)no); put(out, ob.data(), 3 * (size_t)no);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
