// dsdtm_clahe_host.hpp — the entries of include/dsdtm_amd_clahe.h, twice:
//
//   clahe_geometry / clahe_luts_host / clahe_host
//       the same rules (E1-E6 of that header) WITHOUT any device call or library: dependency-free C++ on one thread, every array in host
//       memory. Bit-equal to libdsdtm_amd_clahe.so and to dsdtm_amd/clahe_restatement.py. Compile with -ffp-contract=off (E6 is one
//       order of float operations, each rounded on its own). This is the project's own straightforward C++ (the single-thread baseline of
//       profiles/r27_clahe.txt), not OpenCV's. clahe_geometry (E1, E2 and the three float constants of E5 and E6) is THE definition the
//       library's host side uses too: one function for the device path and the host path.
//   DSDTM::CLAHE
//       the reference drivers' object: DSDTM::CLAHE clahe(3.0, 8, 8); clahe.apply(src, dst) for cv::createCLAHE(3.0, cv::Size(8, 8))
//       ->apply(Image, Image_tmp). on_device = true calls libdsdtm_amd_clahe.so (the context is created at the first apply and kept);
//       false runs clahe_host, for a machine without a device.
// WHICH PATH: see the note at DSDTM::CLAHE below. -DDSDTM_CLAHE_HOST_ONLY leaves out everything that needs the library.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_clahe.h"

namespace DSDTM {

// E1, E2 and the float constants: what both kernels (and both host functions) read of a frame's parameters
struct ClaheGeometry {
    int tiles_x, tiles_y;      // with the default applied
    int ext_w, ext_h;          // the (virtually) extended image
    int tile_w, tile_h, area;
    int clip;                  // 0: no clipping
    float scale;               // 255.0f / (float)area
    float inv_tw, inv_th;      // 1.0f / tile_w, 1.0f / tile_h
};

inline ClaheGeometry clahe_geometry(int width, int height, double clip_limit, int tiles_x, int tiles_y) {
    ClaheGeometry g;
    g.tiles_x = tiles_x ? tiles_x : DSDTM_CLAHE_DEFAULT_TILES; g.tiles_y = tiles_y ? tiles_y : DSDTM_CLAHE_DEFAULT_TILES;
    const bool divides = width % g.tiles_x == 0 && height % g.tiles_y == 0;
    g.ext_w = divides ? width : width + (g.tiles_x - width % g.tiles_x);
    g.ext_h = divides ? height : height + (g.tiles_y - height % g.tiles_y);
    g.tile_w = g.ext_w / g.tiles_x; g.tile_h = g.ext_h / g.tiles_y; g.area = g.tile_w * g.tile_h;
    g.clip = 0;
    if (clip_limit > 0.0) {
        const double q = clip_limit * (double)g.area / 256.0;
        g.clip = q >= (double)g.area ? g.area : (int)q;
        if (g.clip < 1) g.clip = 1;
    }
    g.scale = 255.0f / (float)g.area;
    g.inv_tw = 1.0f / (float)g.tile_w; g.inv_th = 1.0f / (float)g.tile_h;
    return g;
}

namespace clahe_detail {

// BORDER_REFLECT_101 of an index at or beyond 0 (the mirror repeated where the extension is longer than the side less one)
inline int reflect101(int p, int len) {
    while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}
// saturate_u8(cvRound(v)): halves to even (the default rounding mode)
inline uint8_t round_u8(float v) {
    const float r = std::nearbyint(v);
    return r <= 0.0f ? (uint8_t)0 : r >= 255.0f ? (uint8_t)255 : (uint8_t)(int)r;
}
// E6 along one axis: the two clamped tile indices and the weight of the second
inline void axis(int p, float inv, int tiles, int& t1, int& t2, float& a) {
    const float f = (float)p * inv - 0.5f;
    const float fl = std::floor(f);
    a = f - fl;
    const int i = (int)fl;
    t1 = i < 0 ? 0 : i > tiles - 1 ? tiles - 1 : i;          // (the upper clamp never acts: p < width <= ext)
    t2 = i + 1 > tiles - 1 ? tiles - 1 : i + 1;
}

}  // namespace clahe_detail

// E1-E5: luts receives tiles_y * tiles_x tables of 256 bytes, table (ty, tx) at ((ty * tiles_x) + tx) * 256
inline void clahe_luts_host(const uint8_t* src, int src_stride, int width, int height, double clip_limit, int tiles_x, int tiles_y, uint8_t* luts) {
    const ClaheGeometry g = clahe_geometry(width, height, clip_limit, tiles_x, tiles_y);
    std::vector<int> col((size_t)g.ext_w);
    for (int x = 0; x < g.ext_w; ++x) col[(size_t)x] = clahe_detail::reflect101(x, width);
    for (int ty = 0; ty < g.tiles_y; ++ty)
        for (int tx = 0; tx < g.tiles_x; ++tx) {
            int32_t h[256] = {0};
            for (int r = 0; r < g.tile_h; ++r) {
                const uint8_t* row = src + (size_t)clahe_detail::reflect101(ty * g.tile_h + r, height) * (size_t)src_stride;
                for (int c = 0; c < g.tile_w; ++c) ++h[row[col[(size_t)(tx * g.tile_w + c)]]];
            }
            if (g.clip > 0) {
                int32_t clipped = 0;
                for (int i = 0; i < 256; ++i) if (h[i] > g.clip) { clipped += h[i] - g.clip; h[i] = g.clip; }
                const int32_t batch = clipped / 256, residual = clipped - 256 * batch;
                for (int i = 0; i < 256; ++i) h[i] += batch + (i < residual ? 1 : 0);
            }
            uint8_t* lut = luts + ((size_t)ty * (size_t)g.tiles_x + (size_t)tx) * 256;
            int32_t sum = 0;
            for (int i = 0; i < 256; ++i) { sum += h[i]; lut[i] = clahe_detail::round_u8((float)sum * g.scale); }
        }
}

// E6 with given tables
inline void clahe_interpolate_host(const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride, int width, int height, const ClaheGeometry& g,
                                   const uint8_t* luts) {
    std::vector<int> x1((size_t)width), x2((size_t)width);
    std::vector<float> xa((size_t)width);
    for (int x = 0; x < width; ++x) clahe_detail::axis(x, g.inv_tw, g.tiles_x, x1[(size_t)x], x2[(size_t)x], xa[(size_t)x]);
    for (int y = 0; y < height; ++y) {
        int y1, y2;
        float ya;
        clahe_detail::axis(y, g.inv_th, g.tiles_y, y1, y2, ya);
        const uint8_t* l1 = luts + (size_t)y1 * (size_t)g.tiles_x * 256;
        const uint8_t* l2 = luts + (size_t)y2 * (size_t)g.tiles_x * 256;
        const uint8_t* s = src + (size_t)y * (size_t)src_stride;
        uint8_t* d = dst + (size_t)y * (size_t)dst_stride;
        for (int x = 0; x < width; ++x) {
            const int v = s[x];
            const float a = xa[(size_t)x];
            const float w11 = (1.0f - a) * (1.0f - ya), w12 = a * (1.0f - ya), w21 = (1.0f - a) * ya, w22 = a * ya;
            float res = (float)l1[x1[(size_t)x] * 256 + v] * w11;
            res = res + (float)l1[x2[(size_t)x] * 256 + v] * w12;
            res = res + (float)l2[x1[(size_t)x] * 256 + v] * w21;
            res = res + (float)l2[x2[(size_t)x] * 256 + v] * w22;
            d[x] = clahe_detail::round_u8(res);
        }
    }
}

// E1-E6 for one frame. lut_out: NULL, or tiles_y * tiles_x * 256 bytes. dst must not overlap src.
inline void clahe_host(const uint8_t* src, int src_stride, uint8_t* dst, int dst_stride, int width, int height, double clip_limit = DSDTM_CLAHE_DEFAULT_CLIP_LIMIT,
                       int tiles_x = 0, int tiles_y = 0, uint8_t* lut_out = nullptr) {
    const ClaheGeometry g = clahe_geometry(width, height, clip_limit, tiles_x, tiles_y);
    std::vector<uint8_t> own;
    uint8_t* luts = lut_out;
    if (!luts) { own.resize((size_t)g.tiles_x * (size_t)g.tiles_y * 256); luts = own.data(); }
    clahe_luts_host(src, src_stride, width, height, clip_limit, tiles_x, tiles_y, luts);
    clahe_interpolate_host(src, src_stride, dst, dst_stride, width, height, g, luts);
}

// a view of an 8-bit gray image (what the drivers' cv::Mat is to cv::CLAHE::apply): rows of `width` bytes, `stride` bytes apart
struct GrayImage {
    uint8_t* data;
    int width, height, stride;
};

// The reference drivers' object. WHICH PATH. Measured on one MI355X at 640 x 480 (profiles/r27_clahe.txt, wall per call): one frame takes
// the device 27 us from device memory, 45 us from pageable memory into device memory and 72 us from pageable memory with the result read
// back, against 849 us for clahe_host on one host thread; a batch costs 1.7 us per frame at n = 1024. The host function wins nowhere
// measured, so on_device defaults to true; false is for a machine without a device.
class CLAHE {
public:
    explicit CLAHE(double clipLimit = DSDTM_CLAHE_DEFAULT_CLIP_LIMIT, int tilesX = DSDTM_CLAHE_DEFAULT_TILES, int tilesY = DSDTM_CLAHE_DEFAULT_TILES,
                   bool on_device = true, int device = 0)
        : clip_(clipLimit), tx_(tilesX), ty_(tilesY), on_device_(on_device), device_(device) {}
    ~CLAHE() {
#ifndef DSDTM_CLAHE_HOST_ONLY
        dsdtm_clahe_destroy(ctx_);
#endif
    }
    CLAHE(const CLAHE&) = delete;
    CLAHE& operator=(const CLAHE&) = delete;

    // cv::CLAHE::apply(src, dst): dst has src's size and must not overlap it. On the device path either image may lie in host or in
    // device memory (a device dst is ready for dsdtm_frame_prefetch on return); on the host path both lie in host memory.
    void apply(const GrayImage& src, const GrayImage& dst) {
        if (src.width != dst.width || src.height != dst.height) throw std::runtime_error("CLAHE::apply: src and dst differ in size");
        if (!on_device_) {
            if (src.width < DSDTM_CLAHE_MIN_SIDE || src.height < DSDTM_CLAHE_MIN_SIDE || src.width > DSDTM_CLAHE_MAX_SIDE || src.height > DSDTM_CLAHE_MAX_SIDE ||
                tx_ < 0 || ty_ < 0 || tx_ > DSDTM_CLAHE_MAX_TILES || ty_ > DSDTM_CLAHE_MAX_TILES || !std::isfinite(clip_) || clip_ < 0.0 || !src.data || !dst.data ||
                src.stride < src.width || dst.stride < dst.width)
                throw std::runtime_error("CLAHE::apply: what dsdtm_clahe_apply refuses");
            clahe_host(src.data, src.stride, dst.data, dst.stride, src.width, src.height, clip_, tx_, ty_);
            return;
        }
#ifndef DSDTM_CLAHE_HOST_ONLY
        if (!ctx_ && dsdtm_clahe_create(device_, &ctx_) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_clahe_create: ") + dsdtm_clahe_last_error(nullptr));
        dsdtm_clahe_desc d{};
        d.src = src.data; d.dst = dst.data; d.width = src.width; d.height = src.height; d.src_stride = src.stride; d.dst_stride = dst.stride;
        d.clip_limit = clip_; d.tiles_x = tx_; d.tiles_y = ty_;
        if (dsdtm_clahe_apply(ctx_, &d) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_clahe_apply: ") + dsdtm_clahe_last_error(ctx_));
#else
        throw std::runtime_error("CLAHE: built with DSDTM_CLAHE_HOST_ONLY");
#endif
    }
    void setClipLimit(double clipLimit) { clip_ = clipLimit; }
    void setTilesGridSize(int tilesX, int tilesY) { tx_ = tilesX; ty_ = tilesY; }

private:
    double clip_;
    int tx_, ty_;
    bool on_device_;
    int device_;
    dsdtm_clahe_ctx* ctx_ = nullptr;
};

}  // namespace DSDTM
