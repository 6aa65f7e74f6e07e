// undistort.hip — the kernels of libdsdtm_amd_undistort.so (include/dsdtm_amd_undistort.h), gfx950, 64-lane wavefronts.
//
//   undistort_map_kernel      U1: one thread per destination pixel evaluates the forward distortion model in double, every multiply and
//                             add rounded on its own (__dmul_rn / __dadd_rn), and stores the pair (X, Y) at 1/32 pixel with one 8-byte
//                             store. Runs once per map.
//   undistort_frames_kernel   U2 + U3 for n frames in ONE launch: blockIdx.z is the frame, a workgroup of 64 x 4 threads covers 256 x 4
//                             destination pixels, a thread 4 adjacent pixels of a row (a wavefront: 256 adjacent pixels of one row). The
//                             thread's 4 map entries come in as two 16-byte loads (8-byte loads where the row's start is not 16-byte
//                             aligned, and in the tail of a row); the 16 gray taps and 4 depth taps are plain global loads, neighbouring
//                             lanes hitting neighbouring source pixels; the gray result leaves as ONE 32-bit store and the depth result
//                             as ONE 64-bit store where the caller's destination is aligned for it, byte / 16-bit stores otherwise and
//                             in the tail. Integer arithmetic only.
//   undistort_points_kernel   U5: one thread per pixel, five fixed iterations in double, the bearing in newkf.hip's float / double mix.
// No kernel waits for another workgroup, there are no atomics and nothing depends on an order of arrival. Plain C++ only.
#include "undistort.h"

namespace dsdtm {

__device__ __forceinline__ double dm(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double da(double a, double b) { return __dadd_rn(a, b); }

// the terms U1 and U5 share: den = 1 + ((k3*r2 + k2)*r2 + k1)*r2 and the tangential dx, dy
__device__ __forceinline__ void distortion_terms(const UndistortModel& m, double x, double y, double& den, double& dx, double& dy) {
    const double r2 = da(dm(x, x), dm(y, y));
    den = da(1.0, dm(da(dm(da(dm(m.k3, r2), m.k2), r2), m.k1), r2));
    dx = da(dm(dm(dm(2.0, m.p1), x), y), dm(m.p2, da(r2, dm(dm(2.0, x), x))));
    dy = da(dm(m.p1, da(r2, dm(dm(2.0, y), y))), dm(dm(dm(2.0, m.p2), x), y));
}

// cvRound (halves to even: the default rounding mode) saturated to int32; not finite: DSDTM_UNDISTORT_OUTSIDE
__device__ __forceinline__ int32_t round_sat(double v) {
    if (!isfinite(v)) return DSDTM_UNDISTORT_OUTSIDE;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return -2147483647 - 1;
    return (int32_t)rint(v);
}

__global__ __launch_bounds__(256) void undistort_map_kernel(const UndistortModel m, int w, int h, int32_t* __restrict__ map) {
#pragma clang fp contract(off)
    const int u = (int)(blockIdx.x * 64u + threadIdx.x), v = (int)(blockIdx.y * 4u + threadIdx.y);
    if (u >= w || v >= h) return;
    const double x = ((double)u - m.cx) / m.fx, y = ((double)v - m.cy) / m.fy;
    double radial, dx, dy;
    distortion_terms(m, x, y, radial, dx, dy);
    const double xd = da(dm(x, radial), dx), yd = da(dm(y, radial), dy);
    const double mx = da(dm(xd, m.fx), m.cx), my = da(dm(yd, m.fy), m.cy);
    int2 o;
    o.x = round_sat(dm(mx, 32.0)); o.y = round_sat(dm(my, 32.0));
    *reinterpret_cast<int2*>(map + 2 * ((size_t)v * (size_t)w + (size_t)u)) = o;
}

__device__ __forceinline__ uint32_t gray_tap(const uint8_t* __restrict__ src, int stride, int w, int h, int x, int y) {
    return ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) ? (uint32_t)src[(size_t)y * (size_t)stride + (size_t)x] : 0u;
}

__global__ __launch_bounds__(256) void undistort_frames_kernel(const UndistortFrameDev* __restrict__ frames) {
    const UndistortFrameDev f = frames[blockIdx.z];          // (uniform: a copy in scalar registers)
    const int x = (int)(blockIdx.x * 64u + threadIdx.x) * UNDISTORT_PX, y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= f.w || y >= f.h) return;
    const int npx = min((int)UNDISTORT_PX, f.w - x);
    const size_t at = (size_t)y * (size_t)f.w + (size_t)x;
    const int32_t* mp = f.map + 2 * at;
    int32_t X[UNDISTORT_PX] = {0, 0, 0, 0}, Y[UNDISTORT_PX] = {0, 0, 0, 0};
    if (npx == UNDISTORT_PX && (at & 1) == 0) {              // 32 bytes from a 16-byte aligned address
        const int4 a = *reinterpret_cast<const int4*>(mp), b = *reinterpret_cast<const int4*>(mp + 4);
        X[0] = a.x; Y[0] = a.y; X[1] = a.z; Y[1] = a.w; X[2] = b.x; Y[2] = b.y; X[3] = b.z; Y[3] = b.w;
    } else {
#pragma unroll
        for (int k = 0; k < UNDISTORT_PX; ++k)
            if (k < npx) { const int2 a = *reinterpret_cast<const int2*>(mp + 2 * k); X[k] = a.x; Y[k] = a.y; }
    }
    // U2
    uint32_t g[UNDISTORT_PX];
#pragma unroll
    for (int k = 0; k < UNDISTORT_PX; ++k) {
        const int x0 = X[k] >> 5, ax = X[k] & 31, y0 = Y[k] >> 5, ay = Y[k] & 31;
        uint32_t p00 = 0, p01 = 0, p10 = 0, p11 = 0;
        if (k < npx) {
            p00 = gray_tap(f.gray_src, f.gray_src_stride, f.w, f.h, x0, y0); p01 = gray_tap(f.gray_src, f.gray_src_stride, f.w, f.h, x0 + 1, y0);
            p10 = gray_tap(f.gray_src, f.gray_src_stride, f.w, f.h, x0, y0 + 1); p11 = gray_tap(f.gray_src, f.gray_src_stride, f.w, f.h, x0 + 1, y0 + 1);
        }
        g[k] = ((uint32_t)((32 - ax) * (32 - ay)) * p00 + (uint32_t)(ax * (32 - ay)) * p01 + (uint32_t)((32 - ax) * ay) * p10 + (uint32_t)(ax * ay) * p11 + 512u) >> 10;
    }
    uint8_t* drow = f.gray_dst + (size_t)y * (size_t)f.gray_dst_stride + (size_t)x;
    if (npx == UNDISTORT_PX && ((uintptr_t)drow & 3) == 0) {
        *reinterpret_cast<uint32_t*>(drow) = g[0] | (g[1] << 8) | (g[2] << 16) | (g[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < UNDISTORT_PX; ++k) if (k < npx) drow[k] = (uint8_t)g[k];
    }
    // U3
    if (!f.depth_src) return;
    uint32_t d[UNDISTORT_PX];
#pragma unroll
    for (int k = 0; k < UNDISTORT_PX; ++k) {
        const int xn = (X[k] >> 5) + (((X[k] & 31) + 16) >> 5), yn = (Y[k] >> 5) + (((Y[k] & 31) + 16) >> 5);
        d[k] = (k < npx && (unsigned)xn < (unsigned)f.w && (unsigned)yn < (unsigned)f.h)
                   ? (uint32_t)f.depth_src[(size_t)yn * (size_t)f.depth_src_stride + (size_t)xn] : 0u;
    }
    uint16_t* zrow = f.depth_dst + (size_t)y * (size_t)f.depth_dst_stride + (size_t)x;
    if (npx == UNDISTORT_PX && ((uintptr_t)zrow & 7) == 0) {
        uint2 o;
        o.x = d[0] | (d[1] << 16); o.y = d[2] | (d[3] << 16);
        *reinterpret_cast<uint2*>(zrow) = o;
    } else {
#pragma unroll
        for (int k = 0; k < UNDISTORT_PX; ++k) if (k < npx) zrow[k] = (uint16_t)d[k];
    }
}

__global__ __launch_bounds__(256) void undistort_points_kernel(const UndistortModel m, float fxf, float fyf, float cxf, float cyf, int n,
                                                               const float* __restrict__ px_in, const uint8_t* __restrict__ skip,
                                                               float* __restrict__ px_out, double* __restrict__ bearing) {
#pragma clang fp contract(off)
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const float u = px_in[2 * i], v = px_in[2 * i + 1];
    if (skip[i]) { px_out[2 * i] = u; px_out[2 * i + 1] = v; return; }          // mbInitial: the pixel is copied, the bearing stays
    const double x0 = ((double)u - m.cx) / m.fx, y0 = ((double)v - m.cy) / m.fy;
    double x = x0, y = y0;
    for (int it = 0; it < 5; ++it) {
        double den, dx, dy;
        distortion_terms(m, x, y, den, dx, dy);
        const double icdist = 1.0 / den;
        x = dm(x0 - dx, icdist); y = dm(y0 - dy, icdist);
    }
    const float px = (float)da(dm(x, m.fx), m.cx), py = (float)da(dm(y, m.fy), m.cy);
    px_out[2 * i] = px; px_out[2 * i + 1] = py;
    // Frame::Add_Feature's rule (newkf.hip): Pixel2Camera(cv::Point2f, 1.0f) in float, normalised in double
    const float one = 1.0f;
    const double bx = (double)((one * (px - cxf)) / fxf), by = (double)((one * (py - cyf)) / fyf);
    const double nrm = sqrt(bx * bx + by * by + 1.0 * 1.0);
    bearing[3 * (size_t)i] = bx / nrm; bearing[3 * (size_t)i + 1] = by / nrm; bearing[3 * (size_t)i + 2] = 1.0 / nrm;
}

hipError_t undistort_map_launch(const UndistortModel& m, int w, int h, int32_t* map, hipStream_t stream) {
    if (!map || w <= 0 || h <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4), 1);
    hipLaunchKernelGGL(undistort_map_kernel, grid, dim3(64, 4, 1), 0, stream, m, w, h, map);
    return hipGetLastError();
}

hipError_t undistort_frames_launch(const UndistortFrameDev* frames, int n, int max_w, int max_h, hipStream_t stream) {
    if (!frames || n <= 0 || n > DSDTM_UNDISTORT_MAX_FRAMES || max_w <= 0 || max_h <= 0) return hipErrorInvalidValue;
    const int per_block = UNDISTORT_BLOCK_X * UNDISTORT_PX;
    const dim3 grid((unsigned)((max_w + per_block - 1) / per_block), (unsigned)((max_h + UNDISTORT_BLOCK_Y - 1) / UNDISTORT_BLOCK_Y), (unsigned)n);
    hipLaunchKernelGGL(undistort_frames_kernel, grid, dim3(UNDISTORT_BLOCK_X, UNDISTORT_BLOCK_Y, 1), 0, stream, frames);
    return hipGetLastError();
}

hipError_t undistort_points_launch(const UndistortModel& m, float fx, float fy, float cx, float cy, int n, const float* px_in, const uint8_t* skip,
                                   float* px_out, double* bearing, hipStream_t stream) {
    if (n <= 0 || !px_in || !skip || !px_out || !bearing) return hipErrorInvalidValue;
    hipLaunchKernelGGL(undistort_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m, fx, fy, cx, cy, n, px_in, skip, px_out, bearing);
    return hipGetLastError();
}

}  // namespace dsdtm
