// dsdtm_framediff_host.hpp — Moving_Detecter::Mod_FrameDiff (src/Moving_Detection.cpp:36-63) on the host: rules F1-F8 of
// include/dsdtm_amd_framediff.h in plain C++. Header-only; needs neither OpenCV nor any library of this project.
//
//   double M[9];
//   DSDTM::framediff_matrix_host(H, flags, M);                                        // F1; false where the entry refuses
//   DSDTM::warp_perspective_host(b, w, h, b_stride, M, warped, warped_stride);        // F2-F3 (cv::warpPerspective, gray)
//   DSDTM::FrameDiffHost r = DSDTM::frame_diff_host(a, a_stride, b, b_stride, w, h, H, flags, threshold, maxval, mask, mask_stride);
//
// Bit-equal to libdsdtm_amd_framediff.so and to dsdtm_amd/framediff_restatement.py in every byte, M included (tests/test_framediff_cpu.py,
// tests/test_framediff_gpu.py), when compiled without FMA contraction (-ffp-contract=off; the x86-64 default) and without -ffast-math.
// One thread; F6 runs as separable passes over byte images (a rectangle clipped to the image is a product of clipped intervals).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/dsdtm_amd_framediff.h"

namespace DSDTM {

// F1. Returns false for a singular H, an H that is not finite or an inverse that is not.
inline bool framediff_matrix_host(const double H[9], int flags, double M[9]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    for (int k = 0; k < 9; ++k) if (!std::isfinite(H[k])) return false;
    if (flags & DSDTM_FRAMEDIFF_INVERSE_MAP) { std::memcpy(M, H, 9 * sizeof(double)); return true; }
    const double* h = H;
    const double c0 = h[4] * h[8] - h[5] * h[7], c1 = h[3] * h[8] - h[5] * h[6], c2 = h[3] * h[7] - h[4] * h[6];
    const double det = h[0] * c0 - h[1] * c1 + h[2] * c2;
    if (det == 0.0 || !std::isfinite(det)) return false;
    const double d = 1.0 / det;
    const double out[9] = {c0 * d, (h[2] * h[7] - h[1] * h[8]) * d, (h[1] * h[5] - h[2] * h[4]) * d,
                           (h[5] * h[6] - h[3] * h[8]) * d, (h[0] * h[8] - h[2] * h[6]) * d, (h[2] * h[3] - h[0] * h[5]) * d,
                           c2 * d, (h[1] * h[6] - h[0] * h[7]) * d, (h[0] * h[4] - h[1] * h[3]) * d};
    for (int k = 0; k < 9; ++k) if (!std::isfinite(out[k])) return false;
    std::memcpy(M, out, sizeof out);
    return true;
}

// F2's end: NaN is "outside" (-2^31); otherwise clamped to int32 and rounded, halves to even (the default rounding mode)
inline int32_t framediff_round_host(double v) {
    if (v != v) return -2147483647 - 1;
    if (v < -2147483648.0) v = -2147483648.0;
    if (v > 2147483647.0) v = 2147483647.0;
    return (int32_t)std::nearbyint(v);
}

// F2 + F3: b (w x h) seen through M into warped (w x h). warped must not overlap b.
inline void warp_perspective_host(const uint8_t* b, int w, int h, int b_stride, const double M[9], uint8_t* warped, int warped_stride) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    auto tap = [&](int x, int y) -> uint32_t { return ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) ? b[(size_t)y * (size_t)b_stride + (size_t)x] : 0u; };
    for (int y = 0; y < h; ++y) {
        const double yd = (double)y;
        for (int x = 0; x < w; ++x) {
            const double xd = (double)x;
            const double X0 = (M[0] * xd + M[1] * yd) + M[2], Y0 = (M[3] * xd + M[4] * yd) + M[5], W = (M[6] * xd + M[7] * yd) + M[8];
            const double s = W != 0.0 ? 32.0 / W : 0.0;
            const int32_t X = framediff_round_host(X0 * s), Y = framediff_round_host(Y0 * s);
            const int x0 = X >> 5, ax = X & 31, y0 = Y >> 5, ay = Y & 31;
            const uint32_t v = ((uint32_t)((32 - ax) * (32 - ay)) * tap(x0, y0) + (uint32_t)(ax * (32 - ay)) * tap(x0 + 1, y0) +
                                (uint32_t)((32 - ax) * ay) * tap(x0, y0 + 1) + (uint32_t)(ax * ay) * tap(x0 + 1, y0 + 1) + 512u) >> 10;
            warped[(size_t)y * (size_t)warped_stride + (size_t)x] = (uint8_t)v;
        }
    }
}

// one pass of F6 on a packed 0 / 1 image: AND (is_and) or OR over the 5x5 window clipped to the image
inline void framediff_window_host(const std::vector<uint8_t>& src, int w, int h, bool is_and, std::vector<uint8_t>& dst, std::vector<uint8_t>& tmp) {
    tmp.resize(src.size());
    dst.resize(src.size());
    for (int y = 0; y < h; ++y) {
        const uint8_t* s = src.data() + (size_t)y * w;
        uint8_t* t = tmp.data() + (size_t)y * w;
        for (int x = 0; x < w; ++x) {
            const int lo = x - 2 < 0 ? 0 : x - 2, hi = x + 2 >= w ? w - 1 : x + 2;
            uint8_t acc = s[lo];
            for (int i = lo + 1; i <= hi; ++i) acc = is_and ? (acc & s[i]) : (acc | s[i]);
            t[x] = acc;
        }
    }
    for (int y = 0; y < h; ++y) {
        const int lo = y - 2 < 0 ? 0 : y - 2, hi = y + 2 >= h ? h - 1 : y + 2;
        uint8_t* d = dst.data() + (size_t)y * w;
        std::memcpy(d, tmp.data() + (size_t)lo * w, (size_t)w);
        for (int j = lo + 1; j <= hi; ++j) {
            const uint8_t* t = tmp.data() + (size_t)j * w;
            if (is_and) for (int x = 0; x < w; ++x) d[x] &= t[x];
            else for (int x = 0; x < w; ++x) d[x] |= t[x];
        }
    }
}

struct FrameDiffHost {
    bool ok = false;                          // false: F1 refused (nothing written)
    double M[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int32_t n_foreground = 0, n_flagged = 0;
    std::vector<uint8_t> warped, t, e, o, f;  // every stage, packed w x h (t, e, o, f: 0 / 1)
};

// F1-F8 for one pair. mask: NULL or w x h bytes, rows mask_stride apart. features: n_features x 2 floats, every one finite and rounding
// into the image (the entry refuses others); flags: n_features bytes. threshold as given; maxval 0 means DSDTM_FRAMEDIFF_MAXVAL.
inline FrameDiffHost frame_diff_host(const uint8_t* a, int a_stride, const uint8_t* b, int b_stride, int w, int h, const double H[9], int flags,
                                     int threshold, int maxval, uint8_t* mask, int mask_stride, int n_features = 0, const float* feature_px = nullptr,
                                     uint8_t* feature_on_mask = nullptr) {
    FrameDiffHost r;
    if (!framediff_matrix_host(H, flags, r.M)) return r;
    r.ok = true;
    const size_t px = (size_t)w * (size_t)h;
    r.warped.resize(px);
    warp_perspective_host(b, w, h, b_stride, r.M, r.warped.data(), w);
    r.t.resize(px);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int d = (int)a[(size_t)y * (size_t)a_stride + (size_t)x] - (int)r.warped[(size_t)y * w + x];          // F4
            r.t[(size_t)y * w + x] = (d > 0 ? d : 0) > threshold;                                                      // F5
        }
    std::vector<uint8_t> tmp;
    framediff_window_host(r.t, w, h, true, r.e, tmp);
    framediff_window_host(r.e, w, h, false, r.o, tmp);
    framediff_window_host(r.o, w, h, false, r.f, tmp);
    const uint8_t mv = (uint8_t)(maxval ? maxval : DSDTM_FRAMEDIFF_MAXVAL);
    for (size_t i = 0; i < px; ++i) r.n_foreground += r.f[i];
    if (mask)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) mask[(size_t)y * (size_t)mask_stride + (size_t)x] = r.f[(size_t)y * w + x] ? mv : (uint8_t)0;          // F7
    for (int i = 0; i < n_features; ++i) {                                                                             // F8
        const size_t fx = (size_t)std::nearbyintf(feature_px[2 * (size_t)i]), fy = (size_t)std::nearbyintf(feature_px[2 * (size_t)i + 1]);
        const uint8_t on = (r.f[fy * (size_t)w + fx] ? mv : 0) == 255;
        if (feature_on_mask) feature_on_mask[i] = on;
        r.n_flagged += on;
    }
    return r;
}

}  // namespace DSDTM
