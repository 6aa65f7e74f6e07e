// dsdtm_klt_host.hpp — rules K1-K8 of include/dsdtm_amd_klt.h as plain C++ over flat arrays: the pyramid, the grid and the pyramidal
// Lucas-Kanade of KLTWrapper::RunTrack (Thirdparty/fastMCD/src/KLTWrapper.cpp:112-148) and of cv::calcOpticalFlowPyrLK as
// Test/test_Optimizer.cpp:91 calls it. Header-only; needs no library, no OpenCV and no GPU. Bit-equal to dsdtm_amd/klt_restatement.py
// and to libdsdtm_amd_klt.so: every window sum is an int64 sum, the scalar tail of an iteration is IEEE double in the order written in
// the header (build without -ffp-contract=fast and without -ffast-math).
//
//   std::vector<DSDTM::KltLevel> prev = DSDTM::klt_pyramid_host(gray0, w, h, stride, 4, store0), cur = ...;
//   DSDTM::klt_flow_host(prev.data(), cur.data(), 4, n, pts, nullptr, DSDTM::KltParams{}, out_pts, status, iters, residual);
//
// klt_step_host is RunTrack without its last line: it tracks the grid and compacts the survivors in ascending index, A = current,
// B = previous (K9). The H of those correspondences is dsdtm_find_homography's (dsdtm_homography_host.hpp) at a threshold of 1 px: this
// header holds no RANSAC of its own.
//
// DSDTM::KLTWrapper (the end of this file) is the reference's class over the C ABI of libdsdtm_amd_klt.so: Init, RunTrack, GetHomography.
// Only a program that instantiates it links the library; the functions above need nothing.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_klt.h"

namespace DSDTM {

struct KltLevel { const uint8_t* data; int width, height, stride; };
struct KltParams { int window = 10, iterations = 20; double epsilon = 0.03, min_eig = 1e-4; };

inline int klt_reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// K1: `levels` levels; level 0 is the caller's image, the others are written into `store` (which must outlive the result).
inline std::vector<KltLevel> klt_pyramid_host(const uint8_t* image, int width, int height, int stride, int levels, std::vector<std::vector<uint8_t>>& store) {
    std::vector<KltLevel> pyr{KltLevel{image, width, height, stride}};
    store.assign((size_t)(levels > 1 ? levels - 1 : 0), {});
    static const int wk[5] = {1, 4, 6, 4, 1};
    for (int l = 1; l < levels; ++l) {
        const KltLevel s = pyr.back();
        const int dw = (s.width + 1) / 2, dh = (s.height + 1) / 2;
        std::vector<uint8_t>& d = store[(size_t)l - 1];
        d.assign((size_t)dw * dh, 0);
        for (int y = 0; y < dh; ++y)
            for (int x = 0; x < dw; ++x) {
                int acc = 0;
                for (int k = 0; k < 5; ++k) {
                    const uint8_t* row = s.data + (size_t)klt_reflect101(2 * y + k - 2, s.height) * s.stride;
                    int hsum = 0;
                    for (int j = 0; j < 5; ++j) hsum += wk[j] * row[klt_reflect101(2 * x + j - 2, s.width)];
                    acc += wk[k] * hsum;
                }
                d[(size_t)y * dw + x] = (uint8_t)((acc + 128) >> 8);
            }
        pyr.push_back(KltLevel{d.data(), dw, dh, dw});
    }
    return pyr;
}

// K8: the points InitFeatures writes, i major; gw / gh of 0 mean 32 / 24.
inline std::vector<float> klt_grid_host(int width, int height, int gw = 0, int gh = 0) {
    gw = gw ? gw : 32; gh = gh ? gh : 24;
    std::vector<float> p;
    for (int i = 0; i < width / gw - 1; ++i)
        for (int j = 0; j < height / gh - 1; ++j) { p.push_back((float)(i * gw + gw / 2)); p.push_back((float)(j * gh + gh / 2)); }
    return p;
}

namespace klt_detail {
constexpr int W_BITS = 14;
constexpr double SCALE = 1.0 / (1 << 20), FLT_EPS = 1.1920928955078125e-07;

inline void weights(double fx, double fy, int64_t w[4]) {       // K3
    w[0] = (int64_t)std::floor((1.0 - fx) * (1.0 - fy) * 16384.0 + 0.5);
    w[1] = (int64_t)std::floor(fx * (1.0 - fy) * 16384.0 + 0.5);
    w[2] = (int64_t)std::floor((1.0 - fx) * fy * 16384.0 + 0.5);
    w[3] = 16384 - w[0] - w[1] - w[2];
}
inline int64_t px(const KltLevel& L, int x, int y) { return L.data[(size_t)y * L.stride + x]; }
inline int64_t gx(const KltLevel& L, int x, int y) {            // K2
    return 3 * (px(L, x + 1, y - 1) - px(L, x - 1, y - 1)) + 10 * (px(L, x + 1, y) - px(L, x - 1, y)) + 3 * (px(L, x + 1, y + 1) - px(L, x - 1, y + 1));
}
inline int64_t gy(const KltLevel& L, int x, int y) {
    return 3 * (px(L, x - 1, y + 1) - px(L, x - 1, y - 1)) + 10 * (px(L, x, y + 1) - px(L, x, y - 1)) + 3 * (px(L, x + 1, y + 1) - px(L, x + 1, y - 1));
}
template <class F>
inline int64_t tap(F f, const KltLevel& L, int x, int y, const int64_t w[4], int shift) {
    const int64_t s = f(L, x, y) * w[0] + f(L, x + 1, y) * w[1] + f(L, x, y + 1) * w[2] + f(L, x + 1, y + 1) * w[3];
    return (s + ((int64_t)1 << (shift - 1))) >> shift;
}
inline int floor_int(double v) {                                 // floor, held to +-1e6: beyond any level, so `inside` fails there
    const double f = std::floor(v);
    return (int)(f < -1.0e6 ? -1.0e6 : f > 1.0e6 ? 1.0e6 : f);
}
inline bool inside(int ix, int iy, int n, const KltLevel& L, int ring) {      // K4
    return ix - ring >= 0 && iy - ring >= 0 && ix + n + ring <= L.width - 1 && iy + n + ring <= L.height - 1;
}
}  // namespace klt_detail

// K2-K7 for n points. points / guesses (may be null: the points) / out_points: n x 2 floats; status, iterations, residual may be null.
inline void klt_flow_host(const KltLevel* prev, const KltLevel* cur, int levels, int n, const float* points, const float* guesses, const KltParams& P,
                          float* out_points, uint8_t* status, int32_t* iterations, float* residual) {
    using namespace klt_detail;
    const int win = P.window, area = win * win;
    const double half = (win - 1) * 0.5, eps2 = P.epsilon * P.epsilon;
    std::vector<int64_t> Iw((size_t)area), dx((size_t)area), dy((size_t)area);
    for (int k = 0; k < n; ++k) {
        const double top = (double)(1 << (levels - 1));
        const float* g = guesses ? guesses : points;
        double nx = (double)g[2 * k] / top, ny = (double)g[2 * k + 1] / top;
        int used = 0, st = 1;
        double res = 0.0;
        for (int l = levels - 1; l >= 0; --l) {
            const KltLevel &I = prev[l], &J = cur[l];
            const double s = (double)(1 << l);
            const double pxx = (double)points[2 * k] / s - half, pyy = (double)points[2 * k + 1] / s - half;
            const int ix = floor_int(pxx), iy = floor_int(pyy);
            if (l < levels - 1) { nx = nx * 2.0; ny = ny * 2.0; }
            if (!inside(ix, iy, win, I, 1)) { if (l == 0) st = 0; continue; }
            int64_t w[4];
            weights(pxx - std::floor(pxx), pyy - std::floor(pyy), w);
            int64_t A11 = 0, A12 = 0, A22 = 0;
            for (int y = 0; y < win; ++y)
                for (int x = 0; x < win; ++x) {
                    const int i = y * win + x;
                    Iw[i] = tap(px, I, ix + x, iy + y, w, W_BITS - 5);
                    dx[i] = tap(gx, I, ix + x, iy + y, w, W_BITS);
                    dy[i] = tap(gy, I, ix + x, iy + y, w, W_BITS);
                    A11 += dx[i] * dx[i]; A12 += dx[i] * dy[i]; A22 += dy[i] * dy[i];
                }
            const double a11 = (double)A11 * SCALE, a12 = (double)A12 * SCALE, a22 = (double)A22 * SCALE;
            const double det = a11 * a22 - a12 * a12;
            const double min_e = (a22 + a11 - std::sqrt((a11 - a22) * (a11 - a22) + 4.0 * a12 * a12)) / (2.0 * area);
            if (min_e < P.min_eig || det < FLT_EPS) { if (l == 0) st = 0; continue; }
            const double inv = 1.0 / det;
            double qx = nx - half, qy = ny - half, pdx = 0.0, pdy = 0.0;
            for (int j = 0; j < P.iterations; ++j) {
                const int jx = floor_int(qx), jy = floor_int(qy);
                if (!inside(jx, jy, win, J, 0)) { if (l == 0) st = 0; break; }
                int64_t wj[4];
                weights(qx - std::floor(qx), qy - std::floor(qy), wj);
                int64_t B1 = 0, B2 = 0;
                for (int y = 0; y < win; ++y)
                    for (int x = 0; x < win; ++x) {
                        const int i = y * win + x;
                        const int64_t d = tap(px, J, jx + x, jy + y, wj, W_BITS - 5) - Iw[i];
                        B1 += d * dx[i]; B2 += d * dy[i];
                    }
                const double b1 = (double)B1 * SCALE, b2 = (double)B2 * SCALE;
                const double ddx = (a12 * b2 - a22 * b1) * inv, ddy = (a12 * b1 - a11 * b2) * inv;
                qx = qx + ddx; qy = qy + ddy;
                ++used;
                if (ddx * ddx + ddy * ddy <= eps2) break;
                if (j > 0 && std::fabs(ddx + pdx) < 0.01 && std::fabs(ddy + pdy) < 0.01) { qx = qx - ddx * 0.5; qy = qy - ddy * 0.5; break; }
                pdx = ddx; pdy = ddy;
            }
            nx = qx + half; ny = qy + half;
            if (l == 0 && st == 1) {
                const int jx = floor_int(qx), jy = floor_int(qy);
                if (!inside(jx, jy, win, J, 0)) st = 0;
                else {
                    int64_t wj[4], sum = 0;
                    weights(qx - std::floor(qx), qy - std::floor(qy), wj);
                    for (int y = 0; y < win; ++y)
                        for (int x = 0; x < win; ++x) sum += std::llabs(tap(px, J, jx + x, jy + y, wj, W_BITS - 5) - Iw[y * win + x]);
                    res = (double)sum / (32.0 * area);
                }
            }
        }
        out_points[2 * k] = (float)nx; out_points[2 * k + 1] = (float)ny;
        if (status) status[k] = (uint8_t)st;
        if (iterations) iterations[k] = used;
        if (residual) residual[k] = st ? (float)res : 0.0f;
    }
}

struct KltStepHost {
    std::vector<float> prev_points, points;          // the grid and where it went (n_points x 2)
    std::vector<uint8_t> status;
    std::vector<int32_t> iterations;
    std::vector<float> a, b;                         // the survivors in ascending index: A = current, B = previous (n_tracked x 2)
    int n_points = 0, n_tracked = 0;
};

// RunTrack up to the homography: the grid of the level-0 size tracked from `prev` into `cur`, survivors compacted (K8, K9).
inline KltStepHost klt_step_host(const KltLevel* prev, const KltLevel* cur, int levels, int gw = 0, int gh = 0) {
    KltStepHost r;
    r.prev_points = klt_grid_host(prev[0].width, prev[0].height, gw, gh);
    r.n_points = (int)r.prev_points.size() / 2;
    r.points.assign(r.prev_points.size(), 0.0f);
    r.status.assign((size_t)r.n_points, 0);
    r.iterations.assign((size_t)r.n_points, 0);
    klt_flow_host(prev, cur, levels, r.n_points, r.prev_points.data(), nullptr, KltParams{}, r.points.data(), r.status.data(), r.iterations.data(), nullptr);
    for (int k = 0; k < r.n_points; ++k)
        if (r.status[(size_t)k]) {
            r.a.push_back(r.points[2 * k]); r.a.push_back(r.points[2 * k + 1]);
            r.b.push_back(r.prev_points[2 * k]); r.b.push_back(r.prev_points[2 * k + 1]);
            ++r.n_tracked;
        }
    return r;
}

// KLTWrapper (Thirdparty/fastMCD/src/KLTWrapper.h) over the C ABI of include/dsdtm_amd_klt.h. Init(gray) seeds the model, RunTrack(gray)
// tracks the grid from the last image into this one and fits H on the device, GetHomography copies it (9 doubles, row-major, maps the
// current frame to the last one: what Mod_FastMCD takes). No CPU compute path: H is homography.hip's, and this project has no host
// RANSAC outside its tests; a failure throws.
class KLTWrapper {
public:
    explicit KLTWrapper(int device = 0) {
        if (dsdtm_klt_create(device, &ctx_) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_klt_create: ") + dsdtm_klt_last_error(nullptr));
        last_ = dsdtm_klt_result{};
        last_.H[0] = last_.H[4] = last_.H[8] = 1.0;
    }
    ~KLTWrapper() { if (model_) dsdtm_klt_model_destroy(ctx_, model_); dsdtm_klt_destroy(ctx_); }
    KLTWrapper(const KLTWrapper&) = delete;
    KLTWrapper& operator=(const KLTWrapper&) = delete;

    void Init(const uint8_t* gray, int width, int height, int stride) {
        if (model_) { dsdtm_klt_model_destroy(ctx_, model_); model_ = nullptr; }
        check(dsdtm_klt_model_create(ctx_, width, height, 0, &model_), "dsdtm_klt_model_create");
        width_ = width; height_ = height;
        RunTrack(gray, width, height, stride);
    }
    // The first call (or the first with another size) is Init. Returns the step's result (source, n_tracked, n_inliers, ...).
    const dsdtm_klt_result& RunTrack(const uint8_t* gray, int width, int height, int stride) {
        if (!model_ || width != width_ || height != height_) { Init(gray, width, height, stride); return last_; }
        check(dsdtm_klt_step(ctx_, model_, gray, stride, &last_), "dsdtm_klt_step");
        return last_;
    }
    void GetHomography(double H[9]) const { for (int i = 0; i < 9; ++i) H[i] = last_.H[i]; }
    const double* H() const { return last_.H; }
    const dsdtm_klt_result& last() const { return last_; }

private:
    void check(int rc, const char* what) const {
        if (rc != DSDTM_OK) throw std::runtime_error(std::string(what) + ": " + dsdtm_klt_last_error(ctx_));
    }
    dsdtm_klt_ctx* ctx_ = nullptr;
    dsdtm_klt_model* model_ = nullptr;
    int width_ = 0, height_ = 0;
    dsdtm_klt_result last_;
};

}  // namespace DSDTM
