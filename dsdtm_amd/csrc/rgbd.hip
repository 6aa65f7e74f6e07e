// rgbd.hip — the depth half of an RGB-D frame (src/Tracking.cpp:56-57, src/Frame.cpp:35-41): the depth map's way into a
// resident frame, and Frame::Get_FeatureDetph + Frame::UnProject (src/Frame.cpp:152-157, 201-224) as a query on it.
#include "kernels.h"

namespace dsdtm {

// ---- tDImg.convertTo(tDImg, CV_32F, 1.0f / mDepthScale) (src/Tracking.cpp:56) ------------------------------------------
// u16 -> f32 with one float multiply (cv::convertTo's float path for CV_16U -> CV_32F: saturate_cast<float>(src * alpha)).
// The source is usually host-mapped pinned memory: every lane fetches 16 bytes (8 pixels) per trip and the grid is a
// FRACTION of the device — the kernel runs on the prefetch stream beside the tracked frame's kernels, it is bound by the
// link's latency, not by lanes, and workgroups that only wait for the link would take compute units from the frame being
// tracked. `vec`: rows can be moved in 16-byte pieces (source base and row pitch multiples of 16 bytes, destination rows —
// w floats — multiples of 16 bytes); the columns behind the last whole piece, or every column of an image that cannot, go
// through the scalar tail.
typedef unsigned int depth_u32x4 __attribute__((ext_vector_type(4)));
typedef float depth_f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void depth_ingest_kernel(const uint16_t* __restrict__ src, int src_stride, float* __restrict__ dst,
                                                           int w, int h, float inv_scale, int vec) {
    const unsigned tid = blockIdx.x * 256u + threadIdx.x, nthreads = gridDim.x * 256u;
    const unsigned wv = vec ? (unsigned)w / 8u : 0u;           // 16-byte pieces per row
    const unsigned n_vec = wv * (unsigned)h;
    for (unsigned i = tid; i < n_vec; i += nthreads) {
        const unsigned y = i / wv, g = i - y * wv;
        const depth_u32x4 v = __builtin_nontemporal_load((const depth_u32x4*)(src + (size_t)y * src_stride) + g);
        depth_f32x4 lo, hi;
        lo.x = (float)(v.x & 0xffffu) * inv_scale; lo.y = (float)(v.x >> 16) * inv_scale;
        lo.z = (float)(v.y & 0xffffu) * inv_scale; lo.w = (float)(v.y >> 16) * inv_scale;
        hi.x = (float)(v.z & 0xffffu) * inv_scale; hi.y = (float)(v.z >> 16) * inv_scale;
        hi.z = (float)(v.w & 0xffffu) * inv_scale; hi.w = (float)(v.w >> 16) * inv_scale;
        depth_f32x4* o = (depth_f32x4*)(dst + (size_t)y * w) + 2u * g;
        o[0] = lo; o[1] = hi;
    }
    const unsigned x0 = wv * 8u, wt = (unsigned)w - x0;        // the scalar tail: columns x0 .. w-1 of every row
    const unsigned n_tail = wt * (unsigned)h;
    for (unsigned i = tid; i < n_tail; i += nthreads) {
        const unsigned y = i / wt, x = x0 + (i - y * wt);
        dst[(size_t)y * w + x] = (float)src[(size_t)y * src_stride + x] * inv_scale;
    }
}

hipError_t depth_ingest_launch(const uint16_t* src, int src_stride, float* dst, int w, int h, float inv_scale, int num_cus,
                               hipStream_t stream) {
    if (!src || !dst || w <= 0 || h <= 0 || src_stride < w || w > 16384 || h > 16384 || (((size_t)dst) & 15)) return hipErrorInvalidValue;
    const int vec = !(((size_t)src) & 15) && !(src_stride & 7) && !(w & 3) && w >= 8;
    const unsigned items = vec ? (unsigned)(w / 8) * (unsigned)h + (unsigned)(w & 7) * (unsigned)h : (unsigned)w * (unsigned)h;
    // a quarter of the compute units at most (64 of 256: 256 KB of reads in flight per trip)
    unsigned blocks = (items + 255u) / 256u;
    const unsigned cap = num_cus >= 4 ? (unsigned)num_cus / 4u : 1u;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(depth_ingest_kernel, dim3(blocks), dim3(256), 0, stream, src, src_stride, dst, w, h, inv_scale, vec);
    return hipGetLastError();
}

// ---- Frame::Get_FeatureDetph(cv::Point2f) + Frame::UnProject ------------------------------------------------------------
// One thread per pixel: the five depth reads (src/Frame.cpp:201-224; a pixel or neighbour outside the image has no depth —
// the reference indexes the cv::Mat unchecked there), Camera::Pixel2Camera(Point2f, d) in float (src/Camera.cpp:173-178),
// and mT_c2w.inverse() * p in double as Sophus evaluates it: SE3(R^T, -(R^T t)) first, then R^T p + that translation.
__global__ __launch_bounds__(256) void lift_kernel(const LiftArgs a) {
#pragma clang fp contract(off)
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= a.n) return;
    const float px = a.px_xy[2 * i], py = a.px_xy[2 * i + 1];
    const int x = __float2int_rn(px), y = __float2int_rn(py);      // cvRound: to nearest, ties to even
    float d = -1.0f;
    // (a NaN coordinate has no depth: cvRound gives INT_MIN for it, outside every image; the conversion here would give 0)
    if (px == px && py == py && x >= 0 && x < a.w && y >= 0 && y < a.h) {
        const float c = a.depth[(size_t)y * a.w + x];
        if (c != 0.0f) d = c;
        else {
            const int dx[4] = {-1, 0, 1, 0}, dy[4] = {0, -1, 0, 1};
            bool found = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int xx = x + dx[k], yy = y + dy[k];
                if (found || xx < 0 || xx >= a.w || yy < 0 || yy >= a.h) continue;
                const float v = a.depth[(size_t)yy * a.w + xx];
                if (v != 0.0f) { d = v; found = true; }
            }
        }
    }
    a.depth_out[i] = d;
    double pw[3] = {0.0, 0.0, 0.0};
    if (d != -1.0f) {
        const float cxf = d * (px - a.cx) / a.fx, cyf = d * (py - a.cy) / a.fy;
        const double p0 = (double)cxf, p1 = (double)cyf, p2 = (double)d;
        const double* T = a.T;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double rp = T[c] * p0 + T[4 + c] * p1 + T[8 + c] * p2;          // (R^T p)[c]
            const double rt = T[c] * T[3] + T[4 + c] * T[7] + T[8 + c] * T[11];   // (R^T t)[c]
            pw[c] = rp + (-rt);
        }
    }
    a.p_world[3 * i] = pw[0]; a.p_world[3 * i + 1] = pw[1]; a.p_world[3 * i + 2] = pw[2];
}

hipError_t lift_launch(const LiftArgs& args, hipStream_t stream) {
    if (args.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lift_kernel, dim3(((unsigned)args.n + 255u) / 256u), dim3(256), 0, stream, args);
    return hipGetLastError();
}

}  // namespace dsdtm
