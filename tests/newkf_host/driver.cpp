// create_keyframe_host (dsdtm_amd/host/dsdtm_newkf_host.hpp: plain C++, no device call, no library) on the cases tests/newkf_cases.py
// packs; the answers go back as a flat binary file that tests/test_newkf_cpu.py holds against the restatement, integers equal and
// floats / doubles bit-equal. Build: g++ -O2 -std=c++14 -ffp-contract=off. Usage: driver <cases.bin> <answers.bin>
#include <cstdio>
#include <cstdlib>

#include "../../dsdtm_amd/host/dsdtm_newkf_host.hpp"

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
        const std::vector<int32_t> pi = take<int32_t>(7);
        const std::vector<float> pf = take<float>(5);
        dsdtm_newkf_params prm{};
        prm.width = pi[0]; prm.height = pi[1]; prm.cell_size = pi[2]; prm.grid_cols = pi[3]; prm.grid_rows = pi[4]; prm.max_fts = pi[5];
        prm.min_dist = pi[6]; prm.score_floor = pf[0];
        dsdtm_camera cam{};
        cam.fx = pf[1]; cam.fy = pf[2]; cam.cx = pf[3]; cam.cy = pf[4]; cam.width = prm.width; cam.height = prm.height;
        const size_t G = (size_t)prm.grid_cols * (size_t)prm.grid_rows, px = (size_t)prm.width * (size_t)prm.height;
        const std::vector<float> score = take<float>(G);
        const std::vector<int32_t> cx = take<int32_t>(G), cy = take<int32_t>(G), cl = take<int32_t>(G);
        const std::vector<int32_t> head = take<int32_t>(2);
        const size_t ne = (size_t)head[0];
        const std::vector<float> e_px = take<float>(2 * ne);
        const std::vector<int32_t> e_level = take<int32_t>(ne);
        const std::vector<double> e_bearing = take<double>(3 * ne);
        const std::vector<uint8_t> e_has = take<uint8_t>(ne), e_initial = take<uint8_t>(ne);
        const std::vector<int32_t> e_point = take<int32_t>(ne);
        const std::vector<uint16_t> depth = take<uint16_t>(px);
        const float depth_scale = take<float>(1)[0];
        const int32_t has_dyn = take<int32_t>(1)[0];
        const std::vector<uint8_t> dyn = take<uint8_t>(has_dyn ? px : 0);
        const std::vector<double> T = take<double>(12);
        dsdtm_newkf_desc d{};
        d.cell_score = score.data(); d.cell_x = cx.data(); d.cell_y = cy.data(); d.cell_level = cl.data();
        d.n_existing = head[0]; d.first_point_index = head[1];
        d.px_xy = e_px.data(); d.level = e_level.data(); d.bearing = e_bearing.data(); d.has_point = e_has.data(); d.initial = e_initial.data();
        d.point_index = e_point.data();
        d.depth = depth.data(); d.depth_stride = prm.width; d.depth_scale = depth_scale;
        d.dyn_mask = has_dyn ? dyn.data() : nullptr; d.dyn_stride = prm.width;
        d.T_c2w = T.data();
        const DSDTM::NewKeyframeHost o = DSDTM::create_keyframe_host(cam, prm, d);
        const int32_t counts[3] = {o.n_new, o.n_slots, o.n_new_points};
        fwrite(counts, 4, 3, out);
        put(o.point_of_slot); put(o.observes); put(o.px_xy); put(o.level); put(o.bearing); put(o.depth_of_slot); put(o.new_p_world);
    }
    fclose(out);
    return 0;
}
