// example_trackmap.cpp — a track map built incrementally on the device, then dsdtm_track_desc's local-map columns for one pose
// (DSDTM::TrackMap of dsdtm_trackmap_host.hpp over libdsdtm_amd_trackmap.so) filled into a dsdtm_track_desc, beside the host evaluation
// (select_local_map_host + flatten_local_map_host) on the host's copy of the map.
//
//   g++ -O2 -std=c++14 -ffp-contract=off example_trackmap.cpp ../csrc/libdsdtm_amd_trackmap.so -Wl,-rpath,$PWD/../csrc
//       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o example_trackmap          (one command line)
#include <cstdio>
#include <vector>

#include "dsdtm_trackmap_host.hpp"

int main() {
    const dsdtm_camera cam{512.f, 512.f, 320.f, 240.f, 512.f, 640, 480};
    DSDTM::TrackMap map(0);
    std::vector<double> p, T, bearing;
    std::vector<uint8_t> bad, observes;
    std::vector<int32_t> found, n_slots, slots, level;
    std::vector<float> px;
    std::vector<int64_t> off;
    // three keyframes along x, each observing eight points of its own and listing two of its predecessor's: one observed, one whose
    // observation local BA erased while the slot stayed set (observes = 0)
    for (int k = 0; k < 3; ++k) {
        const int first = (int)bad.size();
        for (int i = 0; i < 8; ++i) {
            p.push_back(0.3 * k + 0.05 * i); p.push_back(0.02 * i); p.push_back(2.0 + 0.1 * i);
            bad.push_back(i == 5); found.push_back(1 + i);
        }
        map.WritePoints(first, 8, &p[3 * (size_t)first], &bad[(size_t)first], &found[(size_t)first]);
        std::vector<int32_t> s;
        std::vector<uint8_t> o;
        for (int i = 0; i < 8; ++i) { s.push_back(first + i); o.push_back(1); }
        s.push_back(-1); o.push_back(0);
        if (k) { s.push_back(first - 8); o.push_back(1); s.push_back(first - 7); o.push_back(0); }
        std::vector<float> x;
        std::vector<int32_t> l;
        std::vector<double> b;
        for (size_t i = 0; i < s.size(); ++i) {
            x.push_back(100.f * k + (float)i); x.push_back(7.5f + (float)i); l.push_back((int32_t)(i % 3));
            b.push_back(0.01 * (double)i); b.push_back(-0.02 * k); b.push_back(1.0);
        }
        const double Tk[12] = {1, 0, 0, -0.3 * k, 0, 1, 0, 0, 0, 0, 1, 0};
        map.AddKeyFrame(Tk, (int)s.size(), s.data(), o.data(), x.data(), l.data(), b.data());
        off.push_back((int64_t)slots.size()); n_slots.push_back((int32_t)s.size());
        slots.insert(slots.end(), s.begin(), s.end()); observes.insert(observes.end(), o.begin(), o.end()); T.insert(T.end(), Tk, Tk + 12);
        px.insert(px.end(), x.begin(), x.end()); level.insert(level.end(), l.begin(), l.end()); bearing.insert(bearing.end(), b.begin(), b.end());
    }
    const int32_t hit[2] = {3, 9}, now[2] = {40, 41};       // IncreaseFound of two matched points
    map.WriteFound(2, hit, now);
    found[3] = 40; found[9] = 41;
    const double T_cur[12] = {1, 0, 0, -0.35, 0, 1, 0, 0, 0, 0, 1, 0};
    DSDTM::TrackMap::Columns c;
    map.UpdateLocalMapOnDevice(cam, T_cur, &c, 2, 4);       // (room for 4 observations is too little: asked for again)
    dsdtm_track_desc desc{};
    c.FillDesc(&desc);                                      // desc.kf / desc.T_kf_w: all three keyframes, the caller's
    std::printf("device: %d local keyframes, %d local points, %d observations\n", c.result.n_kf, desc.n_points, c.result.n_obs);
    for (int i = 0; i < desc.n_points; ++i) {
        std::printf("  point %d found %d:", c.point[(size_t)i], desc.mp_found[i]);
        for (int j = desc.obs_offset[i]; j < desc.obs_offset[i + 1]; ++j) std::printf(" (kf %d, px %.1f %.1f)", desc.obs_kf[j], desc.obs_px[2 * j], desc.obs_px[2 * j + 1]);
        std::printf("\n");
    }
    // the same on the host
    DSDTM::TrackMapArrays m;
    m.sel.n_points = (int32_t)bad.size(); m.sel.p_world = p.data(); m.sel.bad = bad.data(); m.sel.n_keyframes = 3; m.sel.T_kf_w = T.data();
    m.sel.n_slots = n_slots.data(); m.sel.slot_offset = off.data(); m.sel.point_of_slot = slots.data();
    m.found = found.data(); m.observes = observes.data(); m.px_xy = px.data(); m.level = level.data(); m.bearing = bearing.data();
    std::vector<int32_t> kf(2), pt(64), pk(64), mf(64), oo(65), ok(256), ol(256);
    std::vector<double> kd(2), mw(192), ob(768);
    std::vector<uint8_t> mb(64);
    std::vector<float> op(512);
    dsdtm_localmap_result r;
    int32_t n_obs = 0;
    DSDTM::select_local_map_host(cam, dsdtm_localmap_params{2, 0}, m.sel, T_cur, kf.data(), kd.data(), 64, pt.data(), pk.data(), &r);
    DSDTM::flatten_local_map_host(m, r.n_points, pt.data(), 256, mw.data(), mf.data(), mb.data(), oo.data(), ok.data(), op.data(), ol.data(), ob.data(), &n_obs);
    pt.resize((size_t)r.n_points); mf.resize((size_t)r.n_points); oo.resize((size_t)r.n_points + 1); ok.resize((size_t)n_obs);
    op.resize(2 * (size_t)n_obs); ob.resize(3 * (size_t)n_obs); mw.resize(3 * (size_t)r.n_points);
    const bool same = n_obs == c.result.n_obs && pt == c.point && mf == c.mp_found && oo == c.obs_offset && ok == c.obs_kf && op == c.obs_px &&
                      ob == c.obs_bearing && mw == c.mp_world;
    std::printf("host: %d local points, %d observations: %s\n", r.n_points, n_obs, same ? "the same" : "DIFFERENT");
    return same ? 0 : 1;
}
