// example_undistort.cpp — a raw (distorted) RGB-D frame on its way into the tracker: cv::undistort, which the reference switched off for its
// cost (src/Frame.cpp:57-61), through DSDTM::Undistorter (libdsdtm_amd_undistort.so) into device memory, then dsdtm_frame_prefetch on
// those device pointers (read in place) and dsdtm_track_frame_on (libdsdtm_amd.so). The frames are generated here: frame 0 becomes the
// reference frame (a grid of features lifted from its rectified depth map), frame 1 is the same scene seen from the same place, so the
// tracked pose must stay the identity. The camera and the coefficients are those of Config/kinect.yaml.
//   build: g++ -std=c++14 example_undistort.cpp -L../csrc -ldsdtm_amd_undistort -ldsdtm_amd -L/opt/rocm/lib -lamdhip64 -o example_undistort
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dsdtm_undistort_host.hpp"

// (the two HIP runtime calls this program makes itself, declared here so that it needs no HIP header: hipError_t is an int, 0 = hipSuccess)
extern "C" int hipMalloc(void** ptr, size_t bytes);
extern "C" int hipFree(void* ptr);

#define HIP_OK(call) do { if ((call) != 0) { std::fprintf(stderr, "%s failed\n", #call); return 1; } } while (0)
#define DSDTM_CHECK(call) do { if ((call) != DSDTM_OK) { std::fprintf(stderr, "%s: %s\n", #call, dsdtm_last_error(ctx)); return 1; } } while (0)

int main() {
    const int W = 640, H = 480, LEVELS = 5;
    dsdtm_camera cam{};
    cam.fx = 517.306408f; cam.fy = 516.469215f; cam.cx = 318.643040f; cam.cy = 255.313989f; cam.f = 525.0f; cam.width = W; cam.height = H;
    const float dist[5] = {0.262383f, -0.953104f, -0.005358f, 0.002628f, 1.163314f};
    // a raw frame: smooth texture, a plane 2 m away (depth_scale 5000)
    std::vector<uint8_t> raw((size_t)W * H);
    std::vector<uint16_t> raw_depth((size_t)W * H, 10000);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) raw[(size_t)y * W + x] = (uint8_t)(128.0 + 60.0 * std::sin(x * 0.11) * std::cos(y * 0.07) + 50.0 * std::sin((x + 2 * y) * 0.031));

    DSDTM::Undistorter und(cam, dist);                   // the map is built once, here
    dsdtm_ctx* ctx = nullptr;
    if (dsdtm_create(0, &ctx) != DSDTM_OK) { std::fprintf(stderr, "dsdtm_create: %s\n", dsdtm_last_error(nullptr)); return 1; }
    uint8_t* d_gray[2] = {nullptr, nullptr};
    uint16_t* d_depth[2] = {nullptr, nullptr};
    dsdtm_frame* frame[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k) {
        HIP_OK(hipMalloc((void**)&d_gray[k], (size_t)W * H));
        HIP_OK(hipMalloc((void**)&d_depth[k], (size_t)W * H * 2));
        // raw frame (pageable host memory) -> rectified frame in device memory; complete when the call returns
        und.rectify(raw.data(), W, d_gray[k], W, raw_depth.data(), W, d_depth[k], W);
        dsdtm_frame_image im{};
        im.gray = d_gray[k]; im.width = W; im.height = H; im.stride = W; im.levels = LEVELS;
        im.depth = d_depth[k]; im.depth_stride = W; im.depth_scale = 5000.0f;
        DSDTM_CHECK(dsdtm_frame_prefetch(ctx, &im, &frame[k]));          // returns at once; reads the device buffers in place
    }
    // the reference frame's features: a grid, lifted from its rectified depth map (Frame::Get_FeatureDetph + UnProject)
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    std::vector<float> px;
    for (int y = 60; y < H - 60; y += 24) for (int x = 80; x < W - 80; x += 24) { px.push_back((float)x); px.push_back((float)y); }
    const int n = (int)px.size() / 2;
    std::vector<float> depth(n);
    std::vector<double> p_world(3 * (size_t)n), bearing(3 * (size_t)n);
    std::vector<uint8_t> initial(n, 1);                      // (every feature has its point: Run aligns those only)
    DSDTM_CHECK(dsdtm_frame_lift(ctx, frame[0], &cam, I, px.data(), n, depth.data(), p_world.data()));
    // (the features sit on the RECTIFIED image already; for features detected on a raw image: und.UndistortFeatures)
    for (int i = 0; i < n; ++i) {
        const double bx = (px[2 * i] - cam.cx) / cam.fx, by = (px[2 * i + 1] - cam.cy) / cam.fy, nrm = std::sqrt(bx * bx + by * by + 1.0);
        bearing[3 * i] = bx / nrm; bearing[3 * i + 1] = by / nrm; bearing[3 * i + 2] = 1.0 / nrm;
    }
    dsdtm_track_desc d{};
    d.image = nullptr; d.width = W; d.height = H; d.stride = W; d.levels = LEVELS;
    d.ref = frame[0]; d.ref_px_xy = px.data(); d.ref_bearing = bearing.data(); d.ref_p_world = p_world.data(); d.ref_initial = initial.data();
    d.n_ref_features = n; d.T_ref_w = I; d.T_seed = I;
    d.align.max_level = LEVELS; d.align.min_level = 0; d.align.max_iters = 10; d.align.min_fts = 15;
    d.min_tracked = 20;
    const int32_t obs_offset[1] = {0};
    d.obs_offset = obs_offset;                            // an empty local map
    d.cell_size = 25; d.max_pyr_levels = LEVELS; d.max_matches = 200; d.align2d_iters = 10; d.pose_opt.max_iterations = 100;
    dsdtm_track_result res{};
    std::vector<dsdtm_track_match> matches(200);
    std::vector<double> rn(200);
    DSDTM_CHECK(dsdtm_track_frame_on(ctx, &cam, &d, frame[1], &res, matches.data(), rn.data()));
    std::printf("tracked %d of %d features; t = (%.2e, %.2e, %.2e)\n", res.n_tracked, n, res.T_run[3], res.T_run[7], res.T_run[11]);
    const bool ok = res.n_tracked >= n / 2 && std::fabs(res.T_run[3]) < 1e-3 && std::fabs(res.T_run[7]) < 1e-3 && std::fabs(res.T_run[11]) < 1e-3;
    for (int k = 0; k < 2; ++k) { dsdtm_frame_destroy(ctx, frame[k]); (void)hipFree(d_gray[k]); (void)hipFree(d_depth[k]); }
    dsdtm_destroy(ctx);
    std::printf("%s\n", ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}
