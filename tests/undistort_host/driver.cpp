// The host functions of dsdtm_amd/host/dsdtm_undistort_host.hpp (undistort_map_host, undistort_frame_host, undistort_points_host) on the
// cases of tests/undistort_cases.py: reads the packed cases, writes the answers (tests/undistort_cases.py: pack / unpack). Needs no
// library and no device. Build with -ffp-contract=off. Test infrastructure (tests/test_undistort_cpu.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../dsdtm_amd/host/dsdtm_undistort_host.hpp"

static std::vector<uint8_t> g_in;
static size_t g_at = 0;
template <class T>
static const T* take(size_t n) {
    const T* p = (const T*)(g_in.data() + g_at);
    g_at += n * sizeof(T);
    if (g_at > g_in.size()) { std::fprintf(stderr, "cases file too short\n"); std::exit(2); }
    return p;
}
template <class T>
static void put(FILE* f, const std::vector<T>& v) { if (!v.empty() && fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(3); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    fseek(fi, 0, SEEK_END);
    g_in.resize((size_t)ftell(fi));
    fseek(fi, 0, SEEK_SET);
    if (fread(g_in.data(), 1, g_in.size(), fi) != g_in.size()) return 2;
    fclose(fi);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    const int32_t* counts = take<int32_t>(2);
    const int n_frames = counts[0], n_points = counts[1];
    for (int c = 0; c < n_frames; ++c) {
        int32_t hd[7];
        memcpy(hd, take<int32_t>(7), sizeof hd);
        float kd[9];
        memcpy(kd, take<float>(9), sizeof kd);
        const int w = hd[0], h = hd[1], has_depth = hd[2], gs = hd[3], gd = hd[4], zs = hd[5], zd = hd[6];
        // exactly-sized copies: an access outside an image is a sanitizer's to see
        const uint8_t* gp = take<uint8_t>((size_t)h * gs);
        std::vector<uint8_t> gray(gp, gp + (size_t)h * gs);
        std::vector<uint16_t> depth;
        if (has_depth) { const uint16_t* p = take<uint16_t>((size_t)h * zs); depth.assign(p, p + (size_t)h * zs); }
        dsdtm_camera cam{};
        cam.fx = kd[0]; cam.fy = kd[1]; cam.cx = kd[2]; cam.cy = kd[3]; cam.width = w; cam.height = h;
        std::vector<int32_t> map((size_t)w * h * 2);
        DSDTM::undistort_map_host(cam, kd + 4, map.data());
        std::vector<uint8_t> gout((size_t)h * gd, 0xA5);
        std::vector<uint16_t> zout(has_depth ? (size_t)h * zd : 0, 0xA5A5);
        DSDTM::undistort_frame_host(map.data(), w, h, gray.data(), gs, gout.data(), gd, has_depth ? depth.data() : nullptr, zs,
                                    has_depth ? zout.data() : nullptr, zd);
        put(fo, map); put(fo, gout); put(fo, zout);
    }
    for (int c = 0; c < n_points; ++c) {
        int32_t hd[2];
        memcpy(hd, take<int32_t>(2), sizeof hd);
        float kd[9];
        memcpy(kd, take<float>(9), sizeof kd);
        const int n = hd[0];
        const float* pp = take<float>(2 * (size_t)n);
        std::vector<float> px(pp, pp + 2 * (size_t)n);
        std::vector<uint8_t> skip;
        if (hd[1]) { const uint8_t* s = take<uint8_t>((size_t)n); skip.assign(s, s + n); }
        dsdtm_camera cam{};
        cam.fx = kd[0]; cam.fy = kd[1]; cam.cx = kd[2]; cam.cy = kd[3]; cam.width = 640; cam.height = 480;
        std::vector<float> out(2 * (size_t)n, -1.0f);
        std::vector<double> bearing(3 * (size_t)n, 7.0);
        DSDTM::undistort_points_host(cam, kd + 4, n, px.data(), hd[1] ? skip.data() : nullptr, out.data(), bearing.data());
        put(fo, out); put(fo, bearing);
    }
    fclose(fo);
    return g_at == g_in.size() ? 0 : 4;
}
