// klt_flow_host, klt_pyramid_host and klt_grid_host (dsdtm_amd/host/dsdtm_klt_host.hpp) behind C entries, for tests/klt_cases.py. Test
// infrastructure only; it links nothing.
#include <cstring>

#include "../../dsdtm_amd/host/dsdtm_klt_host.hpp"

extern "C" int klt_flow_host_c(const uint8_t* prev, int prev_stride, const uint8_t* cur, int cur_stride, int w, int h, int levels, int n, const float* points,
                               const float* guesses, int window, int iterations, double eps, double min_eig, float* out_points, uint8_t* status,
                               int32_t* iters, float* residual) {
    try {
        std::vector<std::vector<uint8_t>> s0, s1;
        const std::vector<DSDTM::KltLevel> p0 = DSDTM::klt_pyramid_host(prev, w, h, prev_stride, levels, s0), p1 = DSDTM::klt_pyramid_host(cur, w, h, cur_stride, levels, s1);
        DSDTM::KltParams P;
        P.window = window; P.iterations = iterations; P.epsilon = eps; P.min_eig = min_eig;
        DSDTM::klt_flow_host(p0.data(), p1.data(), levels, n, points, guesses, P, out_points, status, iters, residual);
        return 0;
    } catch (...) { return -1; }
}

// level `level` of the pyramid of an image into dst (tight rows)
extern "C" int klt_pyramid_host_c(const uint8_t* image, int w, int h, int stride, int level, uint8_t* dst) {
    try {
        std::vector<std::vector<uint8_t>> s;
        const std::vector<DSDTM::KltLevel> p = DSDTM::klt_pyramid_host(image, w, h, stride, level + 1, s);
        const DSDTM::KltLevel& L = p[(size_t)level];
        for (int y = 0; y < L.height; ++y) memcpy(dst + (size_t)y * L.width, L.data + (size_t)y * L.stride, (size_t)L.width);
        return 0;
    } catch (...) { return -1; }
}

// the grid into dst (capacity `cap` points); returns the number of points
extern "C" int klt_grid_host_c(int w, int h, int gw, int gh, float* dst, int cap) {
    const std::vector<float> g = DSDTM::klt_grid_host(w, h, gw, gh);
    const int n = (int)g.size() / 2;
    if (n <= cap && n > 0) memcpy(dst, g.data(), g.size() * sizeof(float));
    return n;
}

// klt_step_host between two images: the survivors (a = current, b = previous, capacity `cap` points each), status per grid point;
// returns n_tracked, *n_points the grid's size
extern "C" int klt_step_host_c(const uint8_t* prev, const uint8_t* cur, int w, int h, int stride, int levels, int gw, int gh, float* a, float* b,
                               uint8_t* status, int cap, int* n_points) {
    try {
        std::vector<std::vector<uint8_t>> s0, s1;
        const std::vector<DSDTM::KltLevel> p0 = DSDTM::klt_pyramid_host(prev, w, h, stride, levels, s0), p1 = DSDTM::klt_pyramid_host(cur, w, h, stride, levels, s1);
        const DSDTM::KltStepHost r = DSDTM::klt_step_host(p0.data(), p1.data(), levels, gw, gh);
        *n_points = r.n_points;
        if (r.n_points > cap) return -1;
        if (r.n_tracked) { memcpy(a, r.a.data(), r.a.size() * sizeof(float)); memcpy(b, r.b.data(), r.b.size() * sizeof(float)); }
        if (r.n_points) memcpy(status, r.status.data(), r.status.size());
        return r.n_tracked;
    } catch (...) { return -1; }
}
