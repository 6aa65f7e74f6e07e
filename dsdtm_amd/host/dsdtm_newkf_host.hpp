// dsdtm_newkf_host.hpp — the entry of include/dsdtm_amd_newkf.h, twice:
//
//   create_keyframe_host
//       the same rules (K1-K6 of that header) on the same dsdtm_newkf_desc, WITHOUT any device call or library: dependency-free C++,
//       every array of the desc in host memory. Integers equal and floats / doubles bit-equal to dsdtm_newkf_make and to
//       dsdtm_amd/keyframe_creation_restatement.py. Compile with -ffp-contract=off.
//   DSDTM::NewKeyframe
//       a thin RAII class over the C ABI (libdsdtm_amd_newkf.so). No CPU compute path: a failure throws.
//   DSDTM::CraeteKeyframeOnDevice / CreateInitialMapRGBDOnDevice
//       the adapters that stand in for Tracking::CraeteKeyframe (src/Tracking.cpp:412-464) and CreateInitialMapRGBD (:147-196) over the
//       classes of dsdtm_host.hpp and DSDTM::Mapping (dsdtm_mapping_host.hpp): Set_ExistingFeatures, dsdtm_detect_cells_frame,
//       dsdtm_newkf_make, points_write + keyframe_add on the resident map, UpdateConnectionOnDevice; the new features are appended to
//       the frame. Link libdsdtm_amd.so, libdsdtm_amd_newkf.so and libdsdtm_amd_mapping.so where they are called.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dsdtm_amd_newkf.h"
#include "dsdtm_host.hpp"
#include "dsdtm_mapping_host.hpp"

namespace DSDTM {

// what dsdtm_newkf_result carries, owned
struct NewKeyframeHost {
    int32_t n_new = 0, n_slots = 0, n_new_points = 0;
    std::vector<int32_t> point_of_slot, level;
    std::vector<uint8_t> observes;
    std::vector<float> px_xy, depth_of_slot;
    std::vector<double> bearing, new_p_world;
};

namespace newkf_detail {

// dy -> half-width of cv::circle(.., radius, .., -1) (OpenCV drawing.cpp Circle(), filled)
inline std::vector<int> circle_half_widths(int radius) {
    std::vector<int> hw((size_t)radius + 2, 0);
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        hw[(size_t)dy] = std::max(hw[(size_t)dy], dx);
        hw[(size_t)dx] = std::max(hw[(size_t)dx], dy);
        dy++; err += plus; plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask; dx += mask; minus -= mask & 2;
    }
    return hw;
}
inline bool in_disc(const std::vector<int>& hw, int radius, long long dx, long long dy) {
    dx = dx < 0 ? -dx : dx; dy = dy < 0 ? -dy : dy;
    return dy <= radius && dx <= hw[(size_t)dy];
}
// cvRound of a finite float: to nearest, halves to even (the default rounding mode)
inline int cv_round(float v) {
    if (v >= 2147483648.0f) return 2147483647;         // saturates, as the kernel's conversion does: far outside every image
    if (v <= -2147483648.0f) return -2147483647 - 1;
    return (int)std::lrintf(v);
}

inline float feature_depth(const dsdtm_newkf_desc& d, int w, int h, float px, float py) {
    const int x = cv_round(px), y = cv_round(py);
    if (x < 0 || x >= w || y < 0 || y >= h) return -1.0f;
    const float inv = 1.0f / d.depth_scale;
    const float c = (float)d.depth[(size_t)y * d.depth_stride + x] * inv;
    if (c != 0.0f) return c;
    const int ox[4] = {-1, 0, 1, 0}, oy[4] = {0, -1, 0, 1};
    for (int k = 0; k < 4; ++k) {
        const int xx = x + ox[k], yy = y + oy[k];
        if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
        const float v = (float)d.depth[(size_t)yy * d.depth_stride + xx] * inv;
        if (v != 0.0f) return v;
    }
    return -1.0f;
}

}  // namespace newkf_detail

// Tracking::CraeteKeyframe from the per-cell corners on (K1-K6). The desc's capacities are not consulted: the vectors grow.
inline NewKeyframeHost create_keyframe_host(const dsdtm_camera& cam, const dsdtm_newkf_params& prm, const dsdtm_newkf_desc& d) {
    using namespace newkf_detail;
    const int W = prm.width, H = prm.height, G = prm.grid_cols * prm.grid_rows, ne = d.n_existing;
    struct New { int x, y, level; };
    std::vector<New> added;
    if (ne < prm.max_fts) {                                                 // K1
        std::vector<int> cand;
        for (int k = 0; k < G; ++k) if (d.cell_score[k] > prm.score_floor) cand.push_back(k);      // (a NaN never passes)
        std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) { return d.cell_score[a] > d.cell_score[b]; });      // K2
        const std::vector<int> hw_min = circle_half_widths(prm.min_dist), hw_cell = circle_half_widths(prm.cell_size);
        std::vector<int> ex, ey;                                            // K3: the centres Set_Mask paints
        if (ne > 0)
            for (int k = 0; k < ne; ++k) if (d.has_point[k]) { ex.push_back(cv_round(d.px_xy[2 * k])); ey.push_back(cv_round(d.px_xy[2 * k + 1])); }
        for (int k : cand) {                                                // K4
            const int x = d.cell_x[k], y = d.cell_y[k], l = d.cell_level[k];
            if (x < 0 || x >= W || y < 0 || y >= H || l < 0 || l > 15) continue;
            bool masked = false;
            for (size_t e = 0; e < ex.size() && !masked; ++e) masked = in_disc(hw_min, prm.min_dist, (long long)x - ex[e], (long long)y - ey[e]);
            if (!masked && ne > 0 && d.dyn_mask) masked = d.dyn_mask[(size_t)y * d.dyn_stride + x] > 200;
            for (size_t e = 0; e < added.size() && !masked; ++e) masked = in_disc(hw_cell, prm.cell_size, x - added[e].x, y - added[e].y);
            if (masked) continue;
            added.push_back({x, y, l});
            if (ne + (int)added.size() >= prm.max_fts) break;
        }
    }
    NewKeyframeHost o;
    o.n_new = (int32_t)added.size(); o.n_slots = ne + o.n_new;
    const size_t S = (size_t)o.n_slots;
    o.point_of_slot.assign(S, -1); o.observes.assign(S, 0); o.level.assign(S, 0); o.px_xy.assign(2 * S, 0.0f);
    o.depth_of_slot.assign(S, -1.0f); o.bearing.assign(3 * S, 0.0);
    for (size_t i = 0; i < S; ++i) {
        bool lift = true;
        if (i < (size_t)ne) {
            o.px_xy[2 * i] = d.px_xy[2 * i]; o.px_xy[2 * i + 1] = d.px_xy[2 * i + 1]; o.level[i] = d.level[i];
            for (int c = 0; c < 3; ++c) o.bearing[3 * i + c] = d.bearing[3 * i + c];
            if (d.initial[i]) { o.point_of_slot[i] = d.point_index[i]; o.observes[i] = 1; lift = false; }       // K6, initial
        } else {                                                            // K5
            const New& f = added[i - (size_t)ne];
            const float px = (float)f.x, py = (float)f.y, one = 1.0f;
            o.px_xy[2 * i] = px; o.px_xy[2 * i + 1] = py; o.level[i] = f.level;
            const double bx = (double)((one * (px - cam.cx)) / cam.fx), by = (double)((one * (py - cam.cy)) / cam.fy);
            const double n = std::sqrt(bx * bx + by * by + 1.0 * 1.0);
            o.bearing[3 * i] = bx / n; o.bearing[3 * i + 1] = by / n; o.bearing[3 * i + 2] = 1.0 / n;
        }
        if (!lift) continue;
        const float px = o.px_xy[2 * i], py = o.px_xy[2 * i + 1];
        const float z = feature_depth(d, W, H, px, py);
        o.depth_of_slot[i] = z;
        if (z < 0.0f) continue;
        const float cxf = z * (px - cam.cx) / cam.fx, cyf = z * (py - cam.cy) / cam.fy;
        const double p0 = (double)cxf, p1 = (double)cyf, p2 = (double)z;
        const double* T = d.T_c2w;
        for (int c = 0; c < 3; ++c) {
            const double rp = T[c] * p0 + T[4 + c] * p1 + T[8 + c] * p2;
            const double rt = T[c] * T[3] + T[4 + c] * T[7] + T[8 + c] * T[11];
            o.new_p_world.push_back(rp + (-rt));
        }
        o.point_of_slot[i] = d.first_point_index + o.n_new_points++;
        o.observes[i] = 1;
    }
    return o;
}

// libdsdtm_amd_newkf.so behind RAII: the context and dsdtm_newkf_make(_batch) on vectors sized to what always fits.
// Which to call (profiles/r20_newkf.txt, one tracker, whole step on a resident frame): detect cells + make 179 us (depth on the device), against
// 190 us for Feature_detector::detect + Frame::Lift; detect cells + create_keyframe_host is about 69 us when the depth image is in host memory.
// In batches make_batch costs 6.9 us per tracker at 64 with resident depth images.
class NewKeyframe {
public:
    explicit NewKeyframe(int device = 0) {
        if (dsdtm_newkf_create(device, &ctx_) != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_newkf_create: ") + dsdtm_newkf_last_error(nullptr));
    }
    ~NewKeyframe() { dsdtm_newkf_destroy(ctx_); }
    NewKeyframe(const NewKeyframe&) = delete;
    NewKeyframe& operator=(const NewKeyframe&) = delete;
    dsdtm_newkf_ctx* handle() const { return ctx_; }

    // the descs' capacities are set here
    std::vector<NewKeyframeHost> make_batch(const dsdtm_camera& cam, const dsdtm_newkf_params& prm, std::vector<dsdtm_newkf_desc> descs) {
        const size_t n = descs.size();
        std::vector<NewKeyframeHost> out(n);
        std::vector<dsdtm_newkf_result> res(n);
        const int G = prm.grid_cols * prm.grid_rows;
        for (size_t t = 0; t < n; ++t) {
            dsdtm_newkf_desc& d = descs[t];
            const size_t S = (size_t)(d.n_existing + std::min(G, std::max(0, prm.max_fts - d.n_existing)));
            d.slot_capacity = d.point_capacity = (int32_t)S; d.bad_capacity = 0;
            NewKeyframeHost& o = out[t];
            o.point_of_slot.resize(S); o.observes.resize(S); o.level.resize(S); o.px_xy.resize(2 * S); o.depth_of_slot.resize(S);
            o.bearing.resize(3 * S); o.new_p_world.resize(3 * S);
            std::memset(&res[t], 0, sizeof res[t]);
            res[t].point_of_slot = o.point_of_slot.data(); res[t].observes = o.observes.data(); res[t].px_xy = o.px_xy.data();
            res[t].level = o.level.data(); res[t].bearing = o.bearing.data(); res[t].depth_of_slot = o.depth_of_slot.data();
            res[t].new_p_world = o.new_p_world.data();
        }
        if (dsdtm_newkf_make_batch(ctx_, &cam, &prm, (int)n, descs.data(), res.data()) != DSDTM_OK)
            throw std::runtime_error(std::string("dsdtm_newkf_make_batch: ") + dsdtm_newkf_last_error(ctx_));
        for (size_t t = 0; t < n; ++t) {
            NewKeyframeHost& o = out[t];
            o.n_new = res[t].n_new; o.n_slots = res[t].n_slots; o.n_new_points = res[t].n_new_points;
            const size_t S = (size_t)o.n_slots, P = (size_t)o.n_new_points;
            o.point_of_slot.resize(S); o.observes.resize(S); o.level.resize(S); o.px_xy.resize(2 * S); o.depth_of_slot.resize(S);
            o.bearing.resize(3 * S); o.new_p_world.resize(3 * P);
        }
        return out;
    }
    NewKeyframeHost make(const dsdtm_camera& cam, const dsdtm_newkf_params& prm, const dsdtm_newkf_desc& desc) {
        return make_batch(cam, prm, std::vector<dsdtm_newkf_desc>(1, desc))[0];
    }

private:
    dsdtm_newkf_ctx* ctx_ = nullptr;
};

// ---- the adapters -----------------------------------------------------------------------------------------------------------------
// Steps 1-3 of CraeteKeyframe on one frame: Set_ExistingFeatures (:415), the image work of detect() (dsdtm_detect_cells_frame on a
// resident frame, dsdtm_detect_cells otherwise) and dsdtm_newkf_make. point_index[k]: feature k's map point as an index of the resident
// map, or -1 (= mvMapPoints[k] == NULL: what Set_Mask reads); a frame whose features carry no point index passes an empty vector.
// depth: the frame's uint16 image, depth_stride ELEMENTS per row, in host, pinned or device memory.
inline NewKeyframeHost DetectAndMakeOnDevice(NewKeyframe& nk, Feature_detector& det, Frame& frame, const std::vector<int32_t>& point_index,
                                             int32_t first_point_index, const uint16_t* depth, int depth_stride, float depth_scale = 5000.0f,
                                             double detection_threshold = 5.0) {
    const size_t ne = frame.mvFeatures.size(), G = det.mvGrid_occupy.size();
    if (!point_index.empty() && point_index.size() != ne) throw std::runtime_error("DetectAndMakeOnDevice: point_index does not match the frame's features");
    det.Set_ExistingFeatures(frame.mvFeatures);
    std::vector<float> score(G);
    std::vector<int32_t> cx(G), cy(G), cl(G);
    const int levels = std::min<int>(det.mPyr_levels, (int)frame.mvImg_Pyr.size());      // (as Feature_detector::detect counts them)
    const dsdtm_detect_params dprm{det.mCell_size, det.mGrid_cols, det.mGrid_rows, levels, 20, (float)detection_threshold};
    int rc;
    if (frame.mDev) rc = dsdtm_detect_cells_frame(detail::ctx(), frame.mDev, det.mvGrid_occupy.data(), &dprm, score.data(), cx.data(), cy.data(), cl.data());
    else {
        const dsdtm_pyramid pyr = detail::to_pyr(frame.mvImg_Pyr);
        rc = dsdtm_detect_cells(detail::ctx(), &pyr, det.mvGrid_occupy.data(), &dprm, score.data(), cx.data(), cy.data(), cl.data());
    }
    det.ResetGrid();                                                        // :152
    if (rc != DSDTM_OK) throw std::runtime_error(std::string("dsdtm_detect_cells: ") + dsdtm_last_error(detail::ctx()));
    std::vector<float> px(2 * ne);
    std::vector<int32_t> level(ne), point(ne, -1);
    std::vector<double> bearing(3 * ne);
    std::vector<uint8_t> has(ne), initial(ne);
    for (size_t k = 0; k < ne; ++k) {
        const Feature& f = frame.mvFeatures[k];
        px[2 * k] = f.mpx_x; px[2 * k + 1] = f.mpx_y; level[k] = f.mlevel; initial[k] = f.mbInitial ? 1 : 0;
        for (int c = 0; c < 3; ++c) bearing[3 * k + c] = f.mNormal[(size_t)c];
        if (!point_index.empty()) point[k] = point_index[k];
        has[k] = point[k] >= 0 ? 1 : 0;
    }
    const Camera& c = *frame.mCamera;
    const dsdtm_camera cam{c.mfx, c.mfy, c.mcx, c.mcy, c.mf, c.mwidth, c.mheight};
    dsdtm_newkf_params prm{};
    prm.width = det.mImg_width; prm.height = det.mImg_height; prm.cell_size = det.mCell_size; prm.grid_cols = det.mGrid_cols;
    prm.grid_rows = det.mGrid_rows; prm.max_fts = det.mMax_fts; prm.min_dist = Config::Min_dist(); prm.score_floor = 20.0f;      // :128
    dsdtm_newkf_desc d{};
    d.cell_score = score.data(); d.cell_x = cx.data(); d.cell_y = cy.data(); d.cell_level = cl.data();
    d.n_existing = (int32_t)ne; d.first_point_index = first_point_index;
    d.px_xy = px.data(); d.level = level.data(); d.bearing = bearing.data(); d.has_point = has.data(); d.initial = initial.data(); d.point_index = point.data();
    d.depth = depth; d.depth_stride = depth_stride; d.depth_scale = depth_scale;
    const Image8& dyn = frame.mDynamicMask;
    if (dyn.cols == prm.width && dyn.rows == prm.height) { d.dyn_mask = dyn.data.data(); d.dyn_stride = dyn.step; }
    d.T_c2w = frame.mT_c2w.m.data();
    return nk.make(cam, prm, d);
}

struct NewKeyframeOutcome {
    bool created = false;                           // false: CreateInitialMapRGBD's test failed (:182); nothing was written
    int32_t kf = -1;                                // the keyframe's index in the resident map
    int32_t first_point_index = 0;                  // the new points are [first_point_index, first_point_index + n_new_points)
    NewKeyframeHost columns;                        // what keyframe_add and points_write were given
    std::vector<std::pair<int32_t, int32_t>> cov;   // mOrderedCovGraph of the new keyframe: (weight, keyframe index), ascending
    int32_t n_connected = 0;
};

// Tracking::CraeteKeyframe on the resident map of `mapping` (stands in for a Tracking method: dsdtm_host.hpp is untouched).
// first_point_index: the map's point count. The frame gets the new features (pixel, level, bearing; mbInitial false) and every lifted
// feature the position of its new point (mMptPose). The caller mirrors the new points and the keyframe on its own objects from
// `columns` (point_of_slot, new_p_world). min_points: see CreateInitialMapRGBDOnDevice.
// Which to call (profiles/r20_newkf.txt): see the comment above NewKeyframe.
inline NewKeyframeOutcome CraeteKeyframeOnDevice(NewKeyframe& nk, Mapping& mapping, Feature_detector& det, Frame& frame,
                                                 const std::vector<int32_t>& point_index, int32_t first_point_index, const uint16_t* depth,
                                                 int depth_stride, float depth_scale = 5000.0f, int min_points = 0) {
    NewKeyframeOutcome out;
    out.first_point_index = first_point_index;
    out.columns = DetectAndMakeOnDevice(nk, det, frame, point_index, first_point_index, depth, depth_stride, depth_scale);
    const NewKeyframeHost& o = out.columns;
    if (o.n_new_points < min_points) return out;
    if (o.n_new_points)                                                     // mMap->AddMapPoint (:453)
        mapping.Check(dsdtm_mapping_points_write(mapping.ctx(), mapping.map(), first_point_index, o.n_new_points, o.new_p_world.data(), nullptr, nullptr),
                      "dsdtm_mapping_points_write");
    int kf = -1;                                                            // mMap->AddKeyFrame (:421)
    mapping.Check(dsdtm_mapping_keyframe_add(mapping.ctx(), mapping.map(), frame.mT_c2w.m.data(), o.n_slots, o.point_of_slot.data(), o.observes.data(),
                                             o.px_xy.data(), o.level.data(), o.bearing.data(), &kf), "dsdtm_mapping_keyframe_add");
    out.kf = kf;
    out.cov = mapping.UpdateConnectionOnDevice(kf, &out.n_connected);       // tKFrame->UpdateConnection() (:459)
    const size_t ne = frame.mvFeatures.size();
    for (size_t i = 0; i < (size_t)o.n_slots; ++i) {
        if (i >= ne) {
            Feature f;
            f.mpx_x = o.px_xy[2 * i]; f.mpx_y = o.px_xy[2 * i + 1]; f.mlevel = o.level[i];
            f.mNormal = {{o.bearing[3 * i], o.bearing[3 * i + 1], o.bearing[3 * i + 2]}};
            frame.mvFeatures.push_back(f);
        }
        const int32_t p = o.point_of_slot[i];
        if (p >= first_point_index && !frame.mvFeatures[i].mbInitial) {     // tFeature->SetPose(tMp) (:450)
            const double* w = &o.new_p_world[3 * (size_t)(p - first_point_index)];
            frame.mvFeatures[i].mMptPose = {{w[0], w[1], w[2]}};
        }
    }
    out.created = true;
    return out;
}

// Tracking::CreateInitialMapRGBD: the same call on a frame without features; fewer than 100 new points (:182): created == false.
inline NewKeyframeOutcome CreateInitialMapRGBDOnDevice(NewKeyframe& nk, Mapping& mapping, Feature_detector& det, Frame& frame, const uint16_t* depth,
                                                       int depth_stride, float depth_scale = 5000.0f) {
    if (!frame.mvFeatures.empty()) throw std::runtime_error("CreateInitialMapRGBDOnDevice: the initial frame has features already");
    return CraeteKeyframeOnDevice(nk, mapping, det, frame, std::vector<int32_t>(), 0, depth, depth_stride, depth_scale, 100);
}

}  // namespace DSDTM
