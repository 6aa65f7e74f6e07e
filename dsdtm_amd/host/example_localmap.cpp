// example_localmap.cpp — a map built incrementally on the device, then the keyframe and point selection of Tracking::UpdateLocalMap
// for one pose (DSDTM::LocalMap of dsdtm_localmap_host.hpp over libdsdtm_amd_localmap.so), beside the host evaluation of the same
// rules (select_local_map_host) on the host's copy of the map.
//
//   g++ -O2 -std=c++14 -ffp-contract=off example_localmap.cpp ../csrc/libdsdtm_amd_localmap.so -Wl,-rpath,$PWD/../csrc
//       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o example_localmap          (one command line)
#include <cstdio>
#include <vector>

#include "dsdtm_localmap_host.hpp"

int main() {
    const dsdtm_camera cam{512.f, 512.f, 320.f, 240.f, 512.f, 640, 480};
    DSDTM::LocalMap map(0);
    std::vector<double> p, T;
    std::vector<uint8_t> bad;
    std::vector<int32_t> n_slots, slots;
    std::vector<int64_t> off;
    // three keyframes along x, each listing eight points of its own in front of it and two of its predecessor's
    for (int k = 0; k < 3; ++k) {
        const int first = (int)bad.size();
        for (int i = 0; i < 8; ++i) { p.push_back(0.3 * k + 0.05 * i); p.push_back(0.02 * i); p.push_back(2.0 + 0.1 * i); bad.push_back(i == 5); }
        map.WritePoints(first, 8, &p[3 * (size_t)first], &bad[(size_t)first]);
        std::vector<int32_t> s;
        for (int i = 0; i < 8; ++i) s.push_back(first + i);
        s.push_back(-1);
        if (k) { s.push_back(first - 8); s.push_back(first - 7); }
        const double Tk[12] = {1, 0, 0, -0.3 * k, 0, 1, 0, 0, 0, 0, 1, 0};
        map.AddKeyFrame(Tk, (int)s.size(), s.data());
        off.push_back((int64_t)slots.size()); n_slots.push_back((int32_t)s.size());
        slots.insert(slots.end(), s.begin(), s.end()); T.insert(T.end(), Tk, Tk + 12);
    }
    const double T_cur[12] = {1, 0, 0, -0.35, 0, 1, 0, 0, 0, 0, 1, 0};
    const DSDTM::LocalMap::Selection s = map.Select(cam, T_cur, 2);
    std::printf("device: %d close, %d local keyframes, %d local points\n", s.result.n_close, s.result.n_kf, s.result.n_points);
    for (size_t j = 0; j < s.kf.size(); ++j) std::printf("  keyframe %d at %.3f\n", s.kf[j], s.kf_dist[j]);
    for (size_t i = 0; i < s.point.size(); ++i) std::printf("  point %d (listed first by local keyframe %d)\n", s.point[i], s.point_kf[i]);
    // the same on the host
    DSDTM::LocalMapArrays m;
    m.n_points = (int32_t)bad.size(); m.p_world = p.data(); m.bad = bad.data(); m.n_keyframes = 3; m.T_kf_w = T.data(); m.n_slots = n_slots.data();
    m.slot_offset = off.data(); m.point_of_slot = slots.data();
    std::vector<int32_t> kf(2), pt(64), pk(64);
    std::vector<double> kd(2);
    dsdtm_localmap_result r;
    DSDTM::select_local_map_host(cam, dsdtm_localmap_params{2, 0}, m, T_cur, kf.data(), kd.data(), 64, pt.data(), pk.data(), &r);
    pt.resize((size_t)r.n_points);
    const bool same = r.n_close == s.result.n_close && r.n_kf == s.result.n_kf && pt == s.point && kd[0] == s.kf_dist[0];
    std::printf("host: %d close, %d local keyframes, %d local points: %s\n", r.n_close, r.n_kf, r.n_points, same ? "the same" : "DIFFERENT");
    // the adapter beside Tracking::TrackFrame, on the caller's object tables (a capacity of 4 is too small: the list is asked for again)
    struct KF { int id; };
    struct MP { int id; };
    std::vector<KF> kf_objects(3);
    std::vector<MP> mp_objects(bad.size());
    std::vector<KF*> all_kfs, local_kfs;
    std::vector<MP*> all_mps, local_mps;
    for (size_t k = 0; k < kf_objects.size(); ++k) { kf_objects[k].id = (int)k; all_kfs.push_back(&kf_objects[k]); }
    for (size_t i = 0; i < mp_objects.size(); ++i) { mp_objects[i].id = (int)i; all_mps.push_back(&mp_objects[i]); }
    map.UpdateLocalMapOnDevice(cam, T_cur, all_kfs, all_mps, &local_kfs, &local_mps, 2, 4);
    bool adapter = local_kfs.size() == s.kf.size() && local_mps.size() == s.point.size();
    for (size_t j = 0; adapter && j < local_kfs.size(); ++j) adapter = local_kfs[j]->id == s.kf[j];
    for (size_t i = 0; adapter && i < local_mps.size(); ++i) adapter = local_mps[i]->id == s.point[i];
    std::printf("adapter: %zu local keyframes (TrackFrame takes all %zu), %zu local points: %s\n", local_kfs.size(), all_kfs.size(), local_mps.size(),
                adapter ? "the same" : "DIFFERENT");
    return same && adapter ? 0 : 1;
}
