// dsdtm_undistort_host.hpp — the entries of include/dsdtm_amd_undistort.h, twice:
//
//   undistort_map_host / undistort_frame_host / undistort_points_host
//       the same rules (U1-U5 of that header) WITHOUT any device call or library: dependency-free C++ on one thread, every array in host
//       memory. Bit-equal to libdsdtm_amd_undistort.so and to dsdtm_amd/undistort_restatement.py. Compile with -ffp-contract=off.
//       This is the project's own straightforward C++ (the single-thread baseline of profiles/r22_undistort.txt), not OpenCV's SIMD remap.
//   DSDTM::Undistorter
//       a thin RAII class over the C ABI (libdsdtm_amd_undistort.so): one context and one map. No CPU compute path: a failure throws.
//       rectify() writes device memory that dsdtm_frame_prefetch reads in place (example_undistort.cpp); UndistortFeatures() stands in
//       for Frame::UndistortFeatures (src/Frame.cpp:94-150) and, for ONE tracker, evaluates undistort_points_host: there the host wins
//       (see the profile), as need_keyframe_host does for the keyframe decision.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_undistort.h"

namespace DSDTM {

namespace undistort_detail {

struct Model { double fx, fy, cx, cy, k1, k2, p1, p2, k3; };
inline Model model(const dsdtm_camera& cam, const float dist[5]) {
    return Model{(double)cam.fx, (double)cam.fy, (double)cam.cx, (double)cam.cy, (double)dist[0], (double)dist[1], (double)dist[2], (double)dist[3], (double)dist[4]};
}
// den = 1 + ((k3 r2 + k2) r2 + k1) r2 and the tangential dx, dy: one rounding per operation (no contraction: see above)
inline void terms(const Model& m, double x, double y, double& den, double& dx, double& dy) {
    const double r2 = x * x + y * y;
    den = 1.0 + ((m.k3 * r2 + m.k2) * r2 + m.k1) * r2;
    dx = ((2.0 * m.p1) * x) * y + m.p2 * (r2 + (2.0 * x) * x);
    dy = m.p1 * (r2 + (2.0 * y) * y) + ((2.0 * m.p2) * x) * y;
}
// cvRound (halves to even: the default rounding mode) saturated to int32; not finite: DSDTM_UNDISTORT_OUTSIDE
inline int32_t round_sat(double v) {
    if (!std::isfinite(v)) return DSDTM_UNDISTORT_OUTSIDE;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return -2147483647 - 1;
    return (int32_t)std::nearbyint(v);
}

}  // namespace undistort_detail

// U1: xy receives cam.width * cam.height pairs (X, Y), row-major
inline void undistort_map_host(const dsdtm_camera& cam, const float dist[5], int32_t* xy) {
    const undistort_detail::Model m = undistort_detail::model(cam, dist);
    for (int v = 0; v < cam.height; ++v)
        for (int u = 0; u < cam.width; ++u) {
            const double x = ((double)u - m.cx) / m.fx, y = ((double)v - m.cy) / m.fy;
            double radial, dx, dy;
            undistort_detail::terms(m, x, y, radial, dx, dy);
            const double xd = x * radial + dx, yd = y * radial + dy;
            const double mx = xd * m.fx + m.cx, my = yd * m.fy + m.cy;
            int32_t* o = xy + 2 * ((size_t)v * (size_t)cam.width + (size_t)u);
            o[0] = undistort_detail::round_sat(mx * 32.0); o[1] = undistort_detail::round_sat(my * 32.0);
        }
}

// U2 + U3 for one frame of w x h; depth_src == NULL: no depth. Strides as in dsdtm_undistort_desc (gray: bytes, depth: elements).
inline void undistort_frame_host(const int32_t* xy, int w, int h, const uint8_t* gray_src, int gray_src_stride, uint8_t* gray_dst, int gray_dst_stride,
                                 const uint16_t* depth_src = nullptr, int depth_src_stride = 0, uint16_t* depth_dst = nullptr, int depth_dst_stride = 0) {
    auto tap = [&](int x, int y) -> uint32_t {
        return ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) ? (uint32_t)gray_src[(size_t)y * (size_t)gray_src_stride + (size_t)x] : 0u;
    };
    for (int v = 0; v < h; ++v)
        for (int u = 0; u < w; ++u) {
            const int32_t X = xy[2 * ((size_t)v * (size_t)w + (size_t)u)], Y = xy[2 * ((size_t)v * (size_t)w + (size_t)u) + 1];
            const int x0 = X >> 5, ax = X & 31, y0 = Y >> 5, ay = Y & 31;
            const uint32_t g = ((uint32_t)((32 - ax) * (32 - ay)) * tap(x0, y0) + (uint32_t)(ax * (32 - ay)) * tap(x0 + 1, y0) +
                                (uint32_t)((32 - ax) * ay) * tap(x0, y0 + 1) + (uint32_t)(ax * ay) * tap(x0 + 1, y0 + 1) + 512u) >> 10;
            gray_dst[(size_t)v * (size_t)gray_dst_stride + (size_t)u] = (uint8_t)g;
            if (!depth_src) continue;
            const int xn = x0 + ((ax + 16) >> 5), yn = y0 + ((ay + 16) >> 5);
            depth_dst[(size_t)v * (size_t)depth_dst_stride + (size_t)u] =
                ((unsigned)xn < (unsigned)w && (unsigned)yn < (unsigned)h) ? depth_src[(size_t)yn * (size_t)depth_src_stride + (size_t)xn] : (uint16_t)0;
        }
}

// U5: px_out may be px_in; skip may be NULL; rows of bearing_out of skipped pixels are not written
inline void undistort_points_host(const dsdtm_camera& cam, const float dist[5], int n, const float* px_in, const uint8_t* skip, float* px_out,
                                  double* bearing_out) {
    const undistort_detail::Model m = undistort_detail::model(cam, dist);
    for (int i = 0; i < n; ++i) {
        const float u = px_in[2 * i], v = px_in[2 * i + 1];
        if (skip && skip[i]) { px_out[2 * i] = u; px_out[2 * i + 1] = v; continue; }
        const double x0 = ((double)u - m.cx) / m.fx, y0 = ((double)v - m.cy) / m.fy;
        double x = x0, y = y0;
        for (int it = 0; it < 5; ++it) {
            double den, dx, dy;
            undistort_detail::terms(m, x, y, den, dx, dy);
            const double icdist = 1.0 / den;
            x = (x0 - dx) * icdist; y = (y0 - dy) * icdist;
        }
        const float px = (float)(x * m.fx + m.cx), py = (float)(y * m.fy + m.cy);
        px_out[2 * i] = px; px_out[2 * i + 1] = py;
        const float one = 1.0f;
        const double bx = (double)((one * (px - cam.cx)) / cam.fx), by = (double)((one * (py - cam.cy)) / cam.fy);
        const double nrm = std::sqrt(bx * bx + by * by + 1.0 * 1.0);
        bearing_out[3 * (size_t)i] = bx / nrm; bearing_out[3 * (size_t)i + 1] = by / nrm; bearing_out[3 * (size_t)i + 2] = 1.0 / nrm;
    }
}

// One camera's rectifier on one device: a context and the map of U1, built once.
class Undistorter {
public:
    Undistorter(const dsdtm_camera& cam, const float dist[5], int device = 0) : cam_(cam) {
        std::memcpy(dist_, dist, sizeof dist_);
        if (dsdtm_undistort_create(device, &ctx_) != DSDTM_OK)
            throw std::runtime_error(std::string("dsdtm_undistort_create: ") + dsdtm_undistort_last_error(nullptr));
        if (dsdtm_undistort_map_create(ctx_, &cam_, dist_, &map_) != DSDTM_OK) {
            const std::string why = dsdtm_undistort_last_error(ctx_);
            dsdtm_undistort_destroy(ctx_);
            throw std::runtime_error("dsdtm_undistort_map_create: " + why);
        }
    }
    ~Undistorter() { dsdtm_undistort_map_destroy(map_); dsdtm_undistort_destroy(ctx_); }
    Undistorter(const Undistorter&) = delete;
    Undistorter& operator=(const Undistorter&) = delete;

    // cv::undistort of one raw frame (depth_src may be NULL, then depth_dst too). Sources: host or device memory; destinations: device
    // memory (ready for dsdtm_frame_prefetch on return) or host memory. Strides as in dsdtm_undistort_desc.
    void rectify(const uint8_t* gray_src, int gray_src_stride, uint8_t* gray_dst, int gray_dst_stride, const uint16_t* depth_src = nullptr,
                 int depth_src_stride = 0, uint16_t* depth_dst = nullptr, int depth_dst_stride = 0) {
        dsdtm_undistort_desc d{};
        d.map = map_; d.gray_src = gray_src; d.gray_dst = gray_dst; d.depth_src = depth_src; d.depth_dst = depth_dst;
        d.gray_src_stride = gray_src_stride; d.gray_dst_stride = gray_dst_stride; d.depth_src_stride = depth_src_stride; d.depth_dst_stride = depth_dst_stride;
        rectify(&d, 1);
    }
    // n frames in ONE submission (descs[i].map: map() of this or of another Undistorter of the same device)
    void rectify(const dsdtm_undistort_desc* descs, int n) {
        if (dsdtm_undistort_frames(ctx_, n, descs) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_undistort_frames: ") + dsdtm_undistort_last_error(ctx_));
    }
    // Frame::UndistortFeatures for one tracker's features (px: n x 2 in place; initial: n flags, mbInitial; bearing: n x 3, rows of
    // initial features untouched): undistort_points_host, which is the faster path for one tracker
    void UndistortFeatures(int n, float* px, const uint8_t* initial, double* bearing) const { undistort_points_host(cam_, dist_, n, px, initial, px, bearing); }
    // the same on the device: worth it when many trackers' features go in one call
    void UndistortFeaturesOnDevice(int n, float* px, const uint8_t* initial, double* bearing) {
        if (dsdtm_undistort_points(ctx_, &cam_, dist_, n, px, initial, px, bearing) != DSDTM_OK)
            throw std::runtime_error(std::string("dsdtm_undistort_points: ") + dsdtm_undistort_last_error(ctx_));
    }
    const dsdtm_undistort_map* map() const { return map_; }
    dsdtm_undistort_ctx* ctx() const { return ctx_; }
    const dsdtm_camera& camera() const { return cam_; }

private:
    dsdtm_camera cam_;
    float dist_[5];
    dsdtm_undistort_ctx* ctx_ = nullptr;
    dsdtm_undistort_map* map_ = nullptr;
};

}  // namespace DSDTM
