// example_newkf.cpp — Tracking::CraeteKeyframe's walk and lift through libdsdtm_amd_newkf.so (include/dsdtm_amd_newkf.h), beside the
// same rules on the host (create_keyframe_host): a synthetic tracker, both answers compared bit for bit.
//   hipcc -std=c++17 -O2 -ffp-contract=off example_newkf.cpp -L../csrc -ldsdtm_amd_newkf -ldsdtm_amd_mapping -ldsdtm_amd -Wl,-rpath,'$ORIGIN/../csrc' -o example_newkf
#include <cstdio>
#include <cstring>

#include "dsdtm_newkf_host.hpp"

// The adapter: one keyframe of a tracker whose frame is resident on the device, into the resident map of `mapping`.
int NewKeyframeStep(DSDTM::NewKeyframe& nk, DSDTM::Mapping& mapping, DSDTM::Feature_detector& det, DSDTM::Frame& frame,
                    const std::vector<int32_t>& point_index, int32_t map_points, const uint16_t* depth) {
    const DSDTM::NewKeyframeOutcome r = DSDTM::CraeteKeyframeOnDevice(nk, mapping, det, frame, point_index, map_points, depth, frame.mCamera->mwidth);
    std::printf("keyframe %d: %d new features, %d new points, %zu covisible keyframes\n", r.kf, r.columns.n_new, r.columns.n_new_points, r.cov.size());
    return map_points + r.columns.n_new_points;
}
bool InitialMap(DSDTM::NewKeyframe& nk, DSDTM::Mapping& mapping, DSDTM::Feature_detector& det, DSDTM::Frame& frame, const uint16_t* depth) {
    return DSDTM::CreateInitialMapRGBDOnDevice(nk, mapping, det, frame, depth, frame.mCamera->mwidth).created;
}

int main() {
    dsdtm_camera cam{525.f, 525.f, 319.5f, 239.5f, 525.f, 640, 480};
    dsdtm_newkf_params prm{};
    prm.width = 640; prm.height = 480; prm.cell_size = 32; prm.grid_cols = 20; prm.grid_rows = 15; prm.max_fts = 400; prm.min_dist = 10; prm.score_floor = 20.f;
    const int G = prm.grid_cols * prm.grid_rows, ne = 40;
    std::vector<float> score((size_t)G), px(2 * (size_t)ne);
    std::vector<int32_t> cx((size_t)G), cy((size_t)G), cl((size_t)G), level((size_t)ne, 0), point((size_t)ne);
    std::vector<uint8_t> has((size_t)ne), initial((size_t)ne);
    std::vector<double> bearing(3 * (size_t)ne, 0.0), T = {1, 0, 0, 0.1, 0, 1, 0, -0.2, 0, 0, 1, 0.3};
    std::vector<uint16_t> depth(640 * 480);
    for (int k = 0; k < G; ++k) {
        score[(size_t)k] = (float)((k * 37) % 90);
        cx[(size_t)k] = (k % prm.grid_cols) * 32 + (k * 7) % 32; cy[(size_t)k] = (k / prm.grid_cols) * 32 + (k * 11) % 32; cl[(size_t)k] = k % 3;
    }
    for (int k = 0; k < ne; ++k) {
        px[2 * (size_t)k] = (float)((k * 97) % 640) + 0.5f; px[2 * (size_t)k + 1] = (float)((k * 61) % 480);
        initial[(size_t)k] = has[(size_t)k] = (uint8_t)(k % 2); point[(size_t)k] = k % 2 ? k : -1; bearing[3 * (size_t)k + 2] = 1.0;
    }
    for (size_t i = 0; i < depth.size(); ++i) depth[i] = (uint16_t)(i % 5 == 0 ? 0 : 4000 + i % 9000);
    dsdtm_newkf_desc d{};
    d.cell_score = score.data(); d.cell_x = cx.data(); d.cell_y = cy.data(); d.cell_level = cl.data();
    d.n_existing = ne; d.first_point_index = 1000;
    d.px_xy = px.data(); d.level = level.data(); d.bearing = bearing.data(); d.has_point = has.data(); d.initial = initial.data(); d.point_index = point.data();
    d.depth = depth.data(); d.depth_stride = 640; d.depth_scale = 5000.f; d.T_c2w = T.data();
    const DSDTM::NewKeyframeHost host = DSDTM::create_keyframe_host(cam, prm, d);
    try {
        DSDTM::NewKeyframe lib(0);
        const DSDTM::NewKeyframeHost dev = lib.make(cam, prm, d);
        const bool same = dev.n_new == host.n_new && dev.n_new_points == host.n_new_points && dev.point_of_slot == host.point_of_slot &&
                          dev.px_xy == host.px_xy && !memcmp(dev.new_p_world.data(), host.new_p_world.data(), host.new_p_world.size() * 8) &&
                          !memcmp(dev.bearing.data(), host.bearing.data(), host.bearing.size() * 8) && dev.depth_of_slot == host.depth_of_slot;
        std::printf("new keyframe: %d existing + %d new features, %d new points; device %s host\n", ne, dev.n_new, dev.n_new_points, same ? "==" : "!=");
        return same ? 0 : 1;
    } catch (const std::exception& e) {
        std::printf("no device path (%s); host: %d new features, %d new points\n", e.what(), host.n_new, host.n_new_points);
        return 2;
    }
}
