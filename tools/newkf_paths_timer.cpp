// The two paths of a new keyframe on ONE tracker, in C++, on a frame that is resident on the device with its depth map (tools/time_newkf.py
// builds and runs this; profiles/r20_newkf.txt):
//   three round trips (the parent commit's path): Feature_detector::detect of dsdtm_host.hpp — dsdtm_detect_cells_frame, then the sort /
//       Set_Mask / walk on one host thread with its full-size mask — then Frame::Lift (dsdtm_frame_lift) for every non-initial feature;
//   the new path: DetectAndMakeOnDevice of dsdtm_newkf_host.hpp — dsdtm_detect_cells_frame, then dsdtm_newkf_make — with the caller's depth
//       image in device, pinned and pageable memory.
// Both start at Set_ExistingFeatures and end with the new features and the lifted points on the host. Medians of `repeats` runs after 3.
//   hipcc -std=c++17 -O2 -ffp-contract=off -I. tools/newkf_paths_timer.cpp -Ldsdtm_amd/csrc -ldsdtm_amd -ldsdtm_amd_newkf -ldsdtm_amd_mapping
// Usage: newkf_paths_timer <scene.bin> <repeats>     scene: int32 w, h, ne; gray w*h u8; depth w*h u16; px 2*ne f32; initial ne u8; T 12 f64
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "dsdtm_amd/host/dsdtm_newkf_host.hpp"

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
static double us(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); }

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 1;
    const int repeats = atoi(argv[2]), warm = 3;
    const std::vector<int32_t> head = take<int32_t>(in, 3);
    const int w = head[0], h = head[1], ne = head[2];
    const std::vector<uint8_t> gray = take<uint8_t>(in, (size_t)w * h);
    const std::vector<uint16_t> depth = take<uint16_t>(in, (size_t)w * h);
    const std::vector<float> px = take<float>(in, 2 * (size_t)ne);
    const std::vector<uint8_t> initial = take<uint8_t>(in, (size_t)ne);
    const std::vector<double> T = take<double>(in, 12);
    using namespace DSDTM;
    Config::CellSize() = 32; Config::Max_fts() = 400; Config::Min_dist() = 10; Config::MaxPyraLevels() = 5;
    CameraPtr cam = std::make_shared<Camera>();
    cam->mfx = 517.3f; cam->mfy = 516.5f; cam->mcx = 318.6f; cam->mcy = 255.3f; cam->mf = 517.3f; cam->mwidth = w; cam->mheight = h;
    Frame fr;
    fr.mCamera = cam;
    fr.mvImg_Pyr.push_back(Image8(w, h));
    fr.mvImg_Pyr[0].data = gray;
    for (int l = 1; l < 5; ++l) fr.mvImg_Pyr.push_back(Image8(w >> l, h >> l));      // (detect() counts the levels here; the pixels are on the device)
    for (int k = 0; k < 12; ++k) fr.mT_c2w.m[(size_t)k] = T[(size_t)k];
    fr.PrefetchOnDevice(5, depth.data(), w, 5000.0f);
    if (dsdtm_frame_wait(detail::ctx(), fr.mDev) != DSDTM_OK) return 3;
    std::vector<Feature> base((size_t)ne);
    std::vector<int32_t> point_index((size_t)ne);
    for (int k = 0; k < ne; ++k) {
        base[(size_t)k].mpx_x = px[2 * (size_t)k]; base[(size_t)k].mpx_y = px[2 * (size_t)k + 1]; base[(size_t)k].mbInitial = initial[(size_t)k] != 0;
        base[(size_t)k].mNormal = {{0.0, 0.0, 1.0}};
        point_index[(size_t)k] = initial[(size_t)k] ? k : -1;            // has_point == mbInitial: the mask detect() of dsdtm_host.hpp paints
    }
    Feature_detector det(w, h);
    typedef std::chrono::steady_clock clk;
    // ---- the three-round-trip path
    std::vector<double> t_detect, t_lift, t_all;
    int n_new_a = 0, n_points_a = 0;
    for (int r = 0; r < repeats + warm; ++r) {
        fr.mvFeatures = base;
        const auto t0 = clk::now();
        det.Set_ExistingFeatures(fr.mvFeatures);
        det.detect(&fr, 5.0);
        const auto t1 = clk::now();
        std::vector<float> lx, ly;
        for (const Feature& f : fr.mvFeatures) if (!f.mbInitial) { lx.push_back(f.mpx_x); ly.push_back(f.mpx_y); }
        std::vector<float> d(lx.size());
        std::vector<double> pw(3 * lx.size());
        if (!lx.empty()) fr.Lift(lx.data(), ly.data(), (int)lx.size(), d.data(), pw.data());
        const auto t2 = clk::now();
        n_new_a = (int)fr.mvFeatures.size() - ne;
        n_points_a = 0;
        for (float v : d) n_points_a += !(v < 0.0f);
        if (r >= warm) { t_detect.push_back(us(t0, t1)); t_lift.push_back(us(t1, t2)); t_all.push_back(us(t0, t2)); }
    }
    // detect cells alone, to split the host walk out of detect()
    std::vector<double> t_cells;
    {
        const size_t G = det.mvGrid_occupy.size();
        std::vector<float> s(G); std::vector<int32_t> x(G), y(G), l(G);
        const dsdtm_detect_params dprm{det.mCell_size, det.mGrid_cols, det.mGrid_rows, 5, 20, 5.0f};
        for (int r = 0; r < repeats + warm; ++r) {
            const auto t0 = clk::now();
            det.Set_ExistingFeatures(base);
            if (dsdtm_detect_cells_frame(detail::ctx(), fr.mDev, det.mvGrid_occupy.data(), &dprm, s.data(), x.data(), y.data(), l.data()) != DSDTM_OK) return 4;
            const auto t1 = clk::now();
            if (r >= warm) t_cells.push_back(us(t0, t1));
        }
        det.ResetGrid();
    }
    printf("three round trips, one host thread: detect() %.1f us (dsdtm_detect_cells_frame %.1f + sort / mask / walk %.1f), Lift of %d pixels %.1f us, "
           "whole path %.1f us; %d cells, %d existing, %d new features, %d new points\n", median(t_detect), median(t_cells), median(t_detect) - median(t_cells),
           n_new_a + (int)std::count(initial.begin(), initial.end(), 0), median(t_lift), median(t_all), (int)det.mvGrid_occupy.size(), ne, n_new_a, n_points_a);
    // ---- the new path, the depth image in each kind of memory
    NewKeyframe nk(0);
    uint16_t *d_dev = nullptr, *d_pin = nullptr;
    const size_t bytes = depth.size() * 2;
    if (hipMalloc((void**)&d_dev, bytes) != hipSuccess || hipHostMalloc((void**)&d_pin, bytes, 0) != hipSuccess) return 5;
    if (hipMemcpy(d_dev, depth.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return 5;
    memcpy(d_pin, depth.data(), bytes);
    const struct { const char* name; const uint16_t* p; } kinds[] = {{"device", d_dev}, {"pinned", d_pin}, {"pageable", depth.data()}};
    int rc = 0;
    for (const auto& k : kinds) {
        std::vector<double> t;
        NewKeyframeHost o;
        for (int r = 0; r < repeats + warm; ++r) {
            fr.mvFeatures = base;
            const auto t0 = clk::now();
            o = DetectAndMakeOnDevice(nk, det, fr, point_index, 1000, k.p, w);
            const auto t1 = clk::now();
            if (r >= warm) t.push_back(us(t0, t1));
        }
        const bool same = o.n_new == n_new_a && o.n_new_points == n_points_a;
        printf("new path (dsdtm_detect_cells_frame + dsdtm_newkf_make), depth in %s memory: %.1f us; %d new features, %d new points%s\n", k.name,
               median(t), o.n_new, o.n_new_points, same ? "" : "  != the three-round-trip path");
        if (!same) rc = 6;
    }
    // ---- the adapters once, untimed: an initial map from the bare image, then a keyframe that carries 40 of its points
    {
        Mapping mapping(0);
        Frame f0;
        f0.mCamera = cam; f0.mvImg_Pyr = fr.mvImg_Pyr; f0.mT_c2w = fr.mT_c2w;
        f0.PrefetchOnDevice(5);
        const NewKeyframeOutcome r0 = CreateInitialMapRGBDOnDevice(nk, mapping, det, f0, d_dev, w);
        std::vector<Feature> carried;
        std::vector<int32_t> carried_point;
        for (size_t i = 0; i < f0.mvFeatures.size() && carried.size() < 40; ++i)
            if (r0.created && r0.columns.point_of_slot[i] >= 0) {
                Feature f = f0.mvFeatures[i];
                f.mbInitial = true;
                carried.push_back(f); carried_point.push_back(r0.columns.point_of_slot[i]);
            }
        fr.mvFeatures = carried;
        const NewKeyframeOutcome r1 = CraeteKeyframeOnDevice(nk, mapping, det, fr, carried_point, r0.columns.n_new_points, d_dev, w);
        const bool ok = r0.created && r0.kf == 0 && r0.columns.n_new_points >= 100 && (int)f0.mvFeatures.size() == r0.columns.n_slots && r1.created &&
                        r1.kf == 1 && r1.columns.n_new > 0 && (int)fr.mvFeatures.size() == r1.columns.n_slots && r1.cov.size() == 1 &&
                        r1.cov[0].first == 40 && r1.cov[0].second == 0 && r1.n_connected == 1;
        printf("adapters: CreateInitialMapRGBDOnDevice keyframe %d with %d points; CraeteKeyframeOnDevice keyframe %d, %d new features, %d new points, "
               "covisibility (%d, %d)%s\n", r0.kf, r0.columns.n_new_points, r1.kf, r1.columns.n_new, r1.columns.n_new_points,
               r1.cov.empty() ? -1 : r1.cov[0].first, r1.cov.empty() ? -1 : r1.cov[0].second, ok ? "" : "  UNEXPECTED");
        if (!ok) rc = 7;
    }
    (void)hipFree(d_dev); (void)hipHostFree(d_pin);
    return rc;
}
