// pose_math.h — Sophus SO3::exp / SO3::log and PoseLocalParameterization::Plus on the [t, log R] parameter block
// (include/Optimizer.h:147, :222-236), shared by the two Ceres restatements: pose_opt.hip (PoseOptimization) and
// local_ba.hip (LocalBundleAdjustment). One restatement, so the two solvers cannot drift apart.
// Internal linkage (anonymous namespace): every kernel file gets its own copy, as when the code lived in pose_opt.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"

namespace dsdtm {

namespace {

// The libm calls of the pose solvers (sincos, atan, log) sit in functions that are NOT inlined: inlined into the
// iteration loop, their ~60 polynomial coefficients are hoisted out of it as loop invariants and held in
// registers for the whole kernel (296 VGPRs, one wave per SIMD); out of line the kernel needs 2/3 of that.
// Scalar in, scalar out: arguments and results travel in registers, nothing goes through the stack.
// (The few-frames instantiation — one frame of the live tracker, one wave per SIMD — has the whole register file
// to itself: there LAT = true inlines them, which saves the call sequences on the iteration's dependent chain.)
__device__ __attribute__((noinline)) double log_out_of_line(double v) { return log(v); }
__device__ __attribute__((noinline)) double atan_out_of_line(double v) { return atan(v); }
struct SinCos { double s, c; };
__device__ __attribute__((noinline)) SinCos sincos_out_of_line(double v) {
    SinCos r;
    sincos(v, &r.s, &r.c);
    return r;
}
template <bool LAT> __device__ __forceinline__ double po_log(double v) { if constexpr (LAT) return log(v); else return log_out_of_line(v); }
template <bool LAT> __device__ __forceinline__ double po_atan(double v) { if constexpr (LAT) return atan(v); else return atan_out_of_line(v); }
template <bool LAT> __device__ __forceinline__ SinCos po_sincos(double v) {
    if constexpr (LAT) { SinCos r; sincos(v, &r.s, &r.c); return r; } else return sincos_out_of_line(v);
}
// x = [t, w] -> SE3(SO3::exp(w), t) (include/Optimizer.h:147). The quaternion part of se3_exp
// (device_math.h) on its own: same series / closed forms, same normalisation, no V matrix.
template <bool LAT>
__device__ __forceinline__ SE3d pose_of(const double* x) {
    const double wx = x[3], wy = x[4], wz = x[5];
    const double theta_sq = wx * wx + wy * wy + wz * wz;
    double ch, imag_factor;
    if (theta_sq < 0.01) {
        const double h2 = 0.25 * theta_sq;
        ch = 1.0 + h2 * (-1.0 / 2 + h2 * (1.0 / 24 + h2 * (-1.0 / 720 + h2 * (1.0 / 40320 + h2 * (-1.0 / 3628800)))));
        const double sinc = 1.0 + h2 * (-1.0 / 6 + h2 * (1.0 / 120 + h2 * (-1.0 / 5040 + h2 * (1.0 / 362880 +
                            h2 * (-1.0 / 39916800)))));
        imag_factor = 0.5 * sinc;
        if (theta_sq < 1e-20) {          // Sophus: theta < SMALL_EPS
            const double theta_po4 = theta_sq * theta_sq;
            imag_factor = 0.5 - 0.0208333 * theta_sq + 0.000260417 * theta_po4;
        }
    } else {
        const double theta = sqrt(theta_sq);
        const SinCos sc = po_sincos<LAT>(0.5 * theta);
        ch = sc.c;
        imag_factor = sc.s * (1.0 / theta);
    }
    SE3d T;
    T.qw = ch; T.qx = imag_factor * wx; T.qy = imag_factor * wy; T.qz = imag_factor * wz;
    quat_normalize(T);
    T.tx = x[0]; T.ty = x[1]; T.tz = x[2];
    return T;
}

// Sophus SO3::log (atan form) of a unit quaternion
template <bool LAT>
__device__ __forceinline__ void so3_log(const SE3d& q, double* w) {
    const double n = sqrt(q.qx * q.qx + q.qy * q.qy + q.qz * q.qz);
    const double qw = q.qw;
    double f;
    if (n < 1e-10) f = 2. / qw - 2. * (n * n) / (qw * (qw * qw));
    else f = 2 * po_atan<LAT>(n / qw) / n;
    w[0] = f * q.qx; w[1] = f * q.qy; w[2] = f * q.qz;
}

// PoseLocalParameterization::Plus (include/Optimizer.h:222-236)
template <bool LAT>
__device__ __forceinline__ void pose_plus(const SE3d& To /* pose_of(x) */, const double* d, double* out) {
    const SE3d Td = pose_of<LAT>(d);
    const SE3d Tn = se3_mul(Td, To);
    out[0] = Tn.tx; out[1] = Tn.ty; out[2] = Tn.tz;
    so3_log<LAT>(Tn, out + 3);
}

}  // namespace

}  // namespace dsdtm
