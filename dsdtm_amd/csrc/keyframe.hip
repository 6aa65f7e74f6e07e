// keyframe.hip — Tracking::NeedKeyframe (reference src/Tracking.cpp:347-410) for n independent trackers in one launch.
//
// One wavefront (= one 64-thread workgroup) per tracker. Lanes stride over the map points (FP64 transform + projection);
// the two order-dependent parts are done without atomics:
//   * K2's "first px_samples non-bad points in list order" is an ORDERED compaction: ballot of the live lanes of a chunk of
//     64 points, position = samples so far + the number of live lanes below — the list order, whatever the timing;
//   * utils::GetMedian (nth_element at floor(m / 2)) is an EXACT k-th-smallest selection on order-preserving 64-bit keys
//     (negative depths order below positive ones), one key bit per pass from the top: count the keys that match the bits
//     decided so far and have a 0 at this bit — integer counts summed over the wave, so the result is a pure function of
//     the multiset: deterministic, no floating-point atomics, and the selected VALUE carries the computed bits unchanged.
// The first lane then evaluates K1, K3 (SE(3) arithmetic of device_math.h / pose_math.h) and K4's walk over the local
// keyframes and stores the verdict with ordinary stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "keyframe.h"

#pragma clang fp contract(off)      // every product and sum rounds on its own, as the host restatements evaluate them (no FMA);
                                    // file scope: also the SE(3) arithmetic of the two headers below
#include "device_math.h"
#include "pose_math.h"

namespace dsdtm {

namespace {

constexpr int KF_LANES = 64;

// double -> unsigned key with the same order (-inf < ... < -0 < +0 < ... < +inf), and back
__device__ __forceinline__ unsigned long long kf_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double kf_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    return __longlong_as_double((long long)b);
}

// the key at index k (0-based) of the ascending order of keys[0 .. m), 0 <= k < m <= the array; all 64 lanes call it
__device__ __forceinline__ unsigned long long kf_kth_smallest(const unsigned long long* keys, int m, int k, int lane) {
    unsigned long long prefix = 0ull, decided = 0ull;
    for (int b = 63; b >= 0; --b) {
        const unsigned long long bit = 1ull << b;
        int c = 0;
        for (int i = lane; i < m; i += KF_LANES) {
            const unsigned long long key = keys[i];
            c += ((key & decided) == prefix && (key & bit) == 0ull) ? 1 : 0;
        }
        c = wave_sum_i32(c);                      // wave-uniform: keys below the candidates that have a 1 here
        if (k >= c) { k -= c; prefix |= bit; }
        decided |= bit;
    }
    return prefix;
}

// T * P as reproject_point (track.hip) evaluates it: row by row, left to right
__device__ __forceinline__ void kf_transform(const double* m, double P0, double P1, double P2, double& x, double& y, double& z) {
    x = m[0] * P0 + m[1] * P1 + m[2] * P2 + m[3];
    y = m[4] * P0 + m[5] * P1 + m[6] * P2 + m[7];
    z = m[8] * P0 + m[9] * P1 + m[10] * P2 + m[11];
}

__global__ __launch_bounds__(KF_LANES) void need_keyframes_kernel(const KeyframeArgs a) {
    __shared__ unsigned long long s_depth[DSDTM_KF_MAX_POINTS];
    __shared__ unsigned long long s_px[KF_LANES];
    const int t = blockIdx.x;
    if (t >= a.n) return;
    const int lane = threadIdx.x;
    const KeyframeTrackerDev& r = ((const KeyframeTrackerDev*)a.blob)[t];
    double Tc[12], Tk[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) { Tc[i] = r.T_cur[i]; Tk[i] = r.T_kf[i]; }
    // the host checked every count; clamped once more because they bound the two LDS arrays
    const int n_cur = min(max(r.n_cur, 0), DSDTM_KF_MAX_POINTS), n_kf = min(max(r.n_kf, 0), DSDTM_KF_MAX_POINTS);
    const int n_lkf = min(max(r.n_lkf, 0), DSDTM_KF_MAX_LOCAL_KF);
    const int samples = min(max(a.prm.px_samples, 1), KF_LANES);
    const unsigned long long below = (1ull << lane) - 1ull;
    const double fx = (double)a.fx, fy = (double)a.fy, cx = (double)a.cx, cy = (double)a.cy;
    bool nonfinite = false;

    // K2 (:359-376): the first `samples` non-bad points of the last keyframe, in list order
    int n_px = 0;
    {
        const double* P = (const double*)(a.blob + r.kf_p);
        const uint8_t* bad = a.blob + r.kf_bad;
        for (int base = 0; base < n_kf && n_px < samples; base += KF_LANES) {
            const int i = base + lane;
            const bool live = i < n_kf && bad[i] == 0;
            const unsigned long long live_mask = __ballot(live);
            const int pos = n_px + __popcll(live_mask & below);
            if (live && pos < samples) {
                const double P0 = P[3 * (size_t)i], P1 = P[3 * (size_t)i + 1], P2 = P[3 * (size_t)i + 2];
                double x, y, z;
                kf_transform(Tc, P0, P1, P2, x, y, z);
                const double u1 = fx * x / z + cx, v1 = fy * y / z + cy;      // Camera::Camera2Pixel (src/Camera.cpp:167-171)
                kf_transform(Tk, P0, P1, P2, x, y, z);
                const double u2 = fx * x / z + cx, v2 = fy * y / z + cy;
                const double du = u1 - u2, dv = v1 - v2;
                const double d = sqrt(du * du + dv * dv);
                s_px[pos] = kf_key(d);
                nonfinite = nonfinite || !isfinite(d);
            }
            n_px += __popcll(live_mask);
        }
        n_px = min(n_px, samples);
    }

    // Frame::Get_SceneDepth (src/Frame.cpp:243-275): the depths of the current frame's non-bad points, and their minimum
    int n_depth = 0;
    double zmin = 1.7976931348623157e308;
    {
        const double* P = (const double*)(a.blob + r.cur_p);
        const uint8_t* bad = a.blob + r.cur_bad;
        for (int base = 0; base < n_cur; base += KF_LANES) {
            const int i = base + lane;
            const bool live = i < n_cur && bad[i] == 0;
            const unsigned long long live_mask = __ballot(live);
            if (live) {
                double x, y, z;
                kf_transform(Tc, P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2], x, y, z);
                s_depth[n_depth + __popcll(live_mask & below)] = kf_key(z);
                zmin = fmin(zmin, z);
                nonfinite = nonfinite || !isfinite(z);
            }
            n_depth += __popcll(live_mask);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) zmin = fmin(zmin, __shfl_xor(zmin, o, KF_LANES));
    }
    __syncthreads();
    const bool undefined = __ballot(nonfinite) != 0ull;
    const double median_px = n_px > 0 ? kf_value(kf_kth_smallest(s_px, n_px, n_px / 2, lane)) : 0.0;
    const double median_depth = n_depth > 0 ? kf_value(kf_kth_smallest(s_depth, n_depth, n_depth / 2, lane)) : 0.0;

    if (lane == 0) {
        dsdtm_keyframe_verdict v;
        int mask = 0;
        if (r.n_valid >= a.prm.min_valid && r.n_valid <= a.prm.max_valid) mask |= 1;          // K1 (:354)
        if (n_px > 0 && median_px > a.prm.min_px_median) mask |= 2;                          // K2 (:378)
        // K3 (:384-390)
        const SE3d D = se3_mul(se3_inverse(se3_from_rt(Tk)), se3_from_rt(Tc));
        double w[3];
        so3_log<true>(D, w);
        const double rot = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        const double trans = sqrt(D.tx * D.tx + D.ty * D.ty + D.tz * D.tz);
        if (rot >= a.prm.min_rot || trans >= a.prm.min_trans) mask |= 4;
        // K4 (:393-402): no absolute value — fabs(a >= b) is the comparison itself
        int svo = -1;
        if (n_depth > 0) {
            const double* C = (const double*)(a.blob + r.lkf);
            const double m = median_depth;
            for (int j = 0; j < n_lkf; ++j) {
                double x, y, z;
                kf_transform(Tc, C[3 * j], C[3 * j + 1], C[3 * j + 2], x, y, z);
                if (x / m >= m && y / m >= m * 0.8 && z / m >= m * 1.3) { svo = j; break; }
            }
        }
        if (svo >= 0) mask |= 8;
        v.need = mask != 0 ? 1 : 0;
        v.reason = (mask & 1) ? 1 : (mask & 2) ? 2 : (mask & 4) ? 3 : (mask & 8) ? 4 : 0;
        v.rule_mask = mask;
        v.undefined = undefined ? 1 : 0;
        v.n_px = n_px; v.n_depth = n_depth; v.svo_kf = svo; v.reserved = 0;
        v.median_px = median_px; v.rot = rot; v.trans = trans;
        v.min_depth = n_depth > 0 ? zmin : 0.0; v.median_depth = median_depth;
        a.verdict[t] = v;
    }
}

}  // namespace

hipError_t need_keyframes_launch(const KeyframeArgs& args, hipStream_t stream) {
    if (args.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(need_keyframes_kernel, dim3((unsigned)args.n), dim3(KF_LANES), 0, stream, args);
    return hipGetLastError();
}

}  // namespace dsdtm
