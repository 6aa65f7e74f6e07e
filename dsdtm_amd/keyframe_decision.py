"""Tracking::NeedKeyframe (reference src/Tracking.cpp:347-410) restated once, in plain float64, line by line — the yardstick
the device entry (dsdtm_need_keyframes, csrc/keyframe.hip) and the host function (need_keyframe_host, host/dsdtm_host.hpp)
are held to. No device, no library call.

Routines it follows: Frame::World2Pixel (src/Frame.cpp:318-323), KeyFrame::World2Pixel (src/Keyframe.cpp:64-69),
Camera::Camera2Pixel (src/Camera.cpp:167-171: float intrinsics promoted to double, fx * x / z + cx, no test on z),
Frame::Get_SceneDepth (src/Frame.cpp:243-275), utils::GetMedian (include/Utils.h:34-40).

Poses are [R|t] (3x4 or 12 doubles, world -> camera). An SE(3) is formed from one as se3_from_rt does (csrc/device_math.h)
and composed as Sophus does (unit quaternion + translation); T * P is evaluated row by row, as reproject_point (csrc/track.hip)
and its Python twin do. Every product and sum rounds on its own (Python floats: no fused multiply-add).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

DBL_MAX = 1.7976931348623157e308


@dataclass
class KeyframeParams:
    """dsdtm_keyframe_params. min_rot / min_trans: KeyFrame.min_rot / KeyFrame.min_trans (src/Tracking.cpp:26-27)."""
    min_valid: int = 30          # :354
    max_valid: int = 50
    px_samples: int = 31         # :374 breaks on size() > 30 AFTER the push: 31 samples, not 30
    min_px_median: float = 40.0  # :378
    min_rot: float = 0.08
    min_trans: float = 0.08


FIELDS = ("need", "reason", "rule_mask", "undefined", "n_px", "n_depth", "svo_kf", "median_px", "rot", "trans", "min_depth",
          "median_depth")


# ---- SE(3) as csrc/device_math.h / csrc/pose_math.h evaluate it ------------------------------------------------------
def _quat_normalize(q):
    qw, qx, qy, qz = q
    n2 = qw * qw + qx * qx + qy * qy + qz * qz
    e = n2 - 1.0
    rn = 1.0 + e * (-0.5 + 0.375 * e) if abs(e) < 1e-5 else 1.0 / math.sqrt(n2)
    return (qw * rn, qx * rn, qy * rn, qz * rn)


def _quat_rotate(q, v):
    qw, qx, qy, qz = q
    vx, vy, vz = v
    ux, uy, uz = qy * vz - qz * vy, qz * vx - qx * vz, qx * vy - qy * vx
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx, cy, cz = qy * uz - qz * uy, qz * ux - qx * uz, qx * uy - qy * ux
    return (vx + qw * ux + cx, vy + qw * uy + cy, vz + qw * uz + cz)


def se3_from_rt(T):
    """[R|t] -> (unit quaternion (w, x, y, z), t): Eigen's rotation-matrix -> quaternion, then normalise."""
    m = [float(v) for v in np.asarray(T, np.float64).reshape(12)]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]
    t = m00 + m11 + m22
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        qw = 0.5 * t
        t = 0.5 / t
        qx, qy, qz = (m21 - m12) * t, (m02 - m20) * t, (m10 - m01) * t
    elif m00 >= m11 and m00 >= m22:
        t = math.sqrt(m00 - m11 - m22 + 1.0)
        qx = 0.5 * t
        t = 0.5 / t
        qw, qy, qz = (m21 - m12) * t, (m10 + m01) * t, (m20 + m02) * t
    elif m11 > m00 and m11 >= m22:
        t = math.sqrt(m11 - m22 - m00 + 1.0)
        qy = 0.5 * t
        t = 0.5 / t
        qw, qz, qx = (m02 - m20) * t, (m21 + m12) * t, (m01 + m10) * t
    else:
        t = math.sqrt(m22 - m00 - m11 + 1.0)
        qz = 0.5 * t
        t = 0.5 / t
        qw, qx, qy = (m10 - m01) * t, (m02 + m20) * t, (m12 + m21) * t
    return _quat_normalize((qw, qx, qy, qz)), (m[3], m[7], m[11])


def se3_inverse(a):
    q, t = a
    qi = (q[0], -q[1], -q[2], -q[3])
    return qi, _quat_rotate(qi, (-t[0], -t[1], -t[2]))


def se3_mul(a, b):
    (aw, ax, ay, az), at = a
    (bw, bx, by, bz), bt = b
    r = _quat_rotate(a[0], bt)
    t = (at[0] + r[0], at[1] + r[1], at[2] + r[2])
    q = (aw * bw - ax * bx - ay * by - az * bz,
         aw * bx + ax * bw + ay * bz - az * by,
         aw * by + ay * bw + az * bx - ax * bz,
         aw * bz + az * bw + ax * by - ay * bx)
    return _quat_normalize(q), t


def so3_log(q):
    """Sophus SO3::log of a unit quaternion, the atan form."""
    qw, qx, qy, qz = q
    n = math.sqrt(qx * qx + qy * qy + qz * qz)
    if n < 1e-10:
        f = 2.0 / qw - 2.0 * (n * n) / (qw * (qw * qw))
    else:
        f = 2 * math.atan(n / qw) / n
    return (f * qx, f * qy, f * qz)


def transform(T12, P):
    """T * P, row by row, left to right."""
    m = T12
    return (m[0] * P[0] + m[1] * P[1] + m[2] * P[2] + m[3],
            m[4] * P[0] + m[5] * P[1] + m[6] * P[2] + m[7],
            m[8] * P[0] + m[9] * P[1] + m[10] * P[2] + m[11])


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def world2pixel(cam, T12, P):
    x, y, z = transform(T12, P)
    fx, fy, cx, cy = (float(np.float32(v)) for v in (cam.fx, cam.fy, cam.cx, cam.cy))
    return (_div(fx * x, z) + cx, _div(fy * y, z) + cy)


def median_index(m: int) -> int:
    """utils::GetMedian: nth_element at begin + floor(size / 2) — for an even size the UPPER middle."""
    return m // 2


def get_median(values):
    """The element at index floor(m / 2) of the ascending order (what nth_element yields there, whatever its algorithm)."""
    return sorted(values)[median_index(len(values))]


def need_keyframe_reference(cam, T_cur_w, T_kf_w, n_valid, cur_p_world, cur_bad, kf_p_world, kf_bad, local_kf_centre,
                            params: KeyframeParams | None = None) -> dict:
    """All four rules of NeedKeyframe, in the reference's order; every one is evaluated.
    cur_p_world / cur_bad : the current frame's map points (n x 3) and their IsBad() (None = none bad)
    kf_p_world / kf_bad   : the last keyframe's map points in mvFeatures order (features without a map point are not in the list)
    local_kf_centre       : Get_CameraCnt() of mvpLocalKeyFrames, n x 3
    Returns a dict of FIELDS, plus px_dist and depths (the two sample lists, in list order)."""
    prm = params or KeyframeParams()
    Tc = [float(v) for v in np.asarray(T_cur_w, np.float64).reshape(12)]
    Tk = [float(v) for v in np.asarray(T_kf_w, np.float64).reshape(12)]
    cur_p = np.asarray(cur_p_world, np.float64).reshape(-1, 3)
    kf_p = np.asarray(kf_p_world, np.float64).reshape(-1, 3)
    lkf = np.asarray(local_kf_centre, np.float64).reshape(-1, 3)
    cur_bad = np.zeros(len(cur_p), np.uint8) if cur_bad is None else np.asarray(cur_bad).reshape(-1)
    kf_bad = np.zeros(len(kf_p), np.uint8) if kf_bad is None else np.asarray(kf_bad).reshape(-1)
    mask = 0
    undefined = False
    # K1 (:352-357)
    if prm.min_valid <= int(n_valid) <= prm.max_valid:
        mask |= 1
    # K2 (:359-381)
    px_dist = []
    for i in range(len(kf_p)):
        if kf_bad[i]:                                              # :365
            continue
        P = [float(v) for v in kf_p[i]]
        u1, v1 = world2pixel(cam, Tc, P)                           # :368
        u2, v2 = world2pixel(cam, Tk, P)                           # :369
        du, dv = u1 - u2, v1 - v2
        px_dist.append(math.sqrt(du * du + dv * dv))               # :372 (sqrt of inf / NaN is inf / NaN)
        if len(px_dist) >= prm.px_samples:                         # :374 (size() > 30 after the push)
            break
    undefined = undefined or any(not math.isfinite(d) for d in px_dist)
    median_px = 0.0
    if px_dist and not undefined:
        median_px = get_median(px_dist)                            # :377
        if median_px > prm.min_px_median:                          # :378
            mask |= 2
    # K3 (:383-390)
    D = se3_mul(se3_inverse(se3_from_rt(Tk)), se3_from_rt(Tc))
    w = so3_log(D[0])
    rot = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    trans = math.sqrt(D[1][0] * D[1][0] + D[1][1] * D[1][1] + D[1][2] * D[1][2])
    if rot >= prm.min_rot or trans >= prm.min_trans:
        mask |= 4
    # K4 (:392-402)
    depths = []
    min_depth = DBL_MAX
    for i in range(len(cur_p)):
        if cur_bad[i]:
            continue
        z = transform(Tc, [float(v) for v in cur_p[i]])[2]
        depths.append(z)
        min_depth = float(np.fmin(min_depth, z))
    undefined = undefined or any(not math.isfinite(z) for z in depths)
    svo_kf, median_depth = -1, 0.0
    if depths and not undefined:
        m = median_depth = get_median(depths)
        for j in range(len(lkf)):
            c = transform(Tc, [float(v) for v in lkf[j]])
            # fabs(a >= b) is the comparison itself (:398-400): no absolute value
            if _div(c[0], m) >= m and _div(c[1], m) >= m * 0.8 and _div(c[2], m) >= m * 1.3:
                svo_kf = j
                break
    if svo_kf >= 0:
        mask |= 8
    reason = 1 if mask & 1 else 2 if mask & 2 else 3 if mask & 4 else 4 if mask & 8 else 0
    return dict(need=int(mask != 0), reason=reason, rule_mask=mask, undefined=int(undefined), n_px=len(px_dist),
                n_depth=len(depths), svo_kf=svo_kf, median_px=median_px, rot=rot, trans=trans,
                min_depth=min_depth if depths else 0.0, median_depth=median_depth, px_dist=px_dist, depths=depths)
