"""Tracking::GetCloseKeyFrames (reference src/Tracking.cpp:315-345) and the keyframe and point selection of
Tracking::UpdateLocalMap (:258-297) restated once, in plain Python floats (float64), operation by operation — the yardstick the
device entry (dsdtm_localmap_select, csrc/localmap.hip) and the host function (select_local_map_host,
host/dsdtm_localmap_host.hpp) are held to. No device, no library call. The rules are L1-L4 of include/dsdtm_amd_localmap.h.

A map is a dict of arrays: p_world (P x 3), bad (P), T_kf_w (K x 12, [R|t] row-major, world -> camera) and slots (a list of K int
arrays: KeyFrame::mvMapPoints as point indices, -1 = NULL). The camera has float32 members (fx, fy, cx, cy) and width, height.
Every product and sum rounds on its own (Python floats: no fused multiply-add).
"""
from __future__ import annotations

import math

import numpy as np


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def cv_round(v: float) -> int:
    """cvRound of a cv::Point2f member: the double is narrowed to float FIRST, then rounded half to even."""
    return int(np.rint(np.float64(np.float32(v))))


def in_image(cam, x: float, y: float, boundary: int) -> bool:
    """Camera::IsInImage(cv::Point2f(x, y), boundary, 0) (src/Camera.cpp:187-193); not finite or |.| >= 1e9: not in the image."""
    if not (abs(x) < 1e9) or not (abs(y) < 1e9):
        return False
    xr, yr = cv_round(x), cv_round(y)
    return boundary <= xr < int(cam.width) - boundary and boundary <= yr < int(cam.height) - boundary


def intrinsics(cam):
    """The camera's float members promoted to double (src/Camera.cpp:167-171)."""
    return tuple(float(np.float32(v)) for v in (cam.fx, cam.fy, cam.cx, cam.cy))


def is_visible(cam, T12, X, boundary: int = 0, intr=None) -> bool:
    """Frame::isVisible (src/Frame.cpp:300-311). intr: intrinsics(cam), for a caller that has them already."""
    m = T12
    x = m[0] * X[0] + m[1] * X[1] + m[2] * X[2] + m[3]
    y = m[4] * X[0] + m[5] * X[1] + m[6] * X[2] + m[7]
    z = m[8] * X[0] + m[9] * X[1] + m[10] * X[2] + m[11]
    if z < 0.0:                                                     # src/Frame.cpp:303
        return False
    fx, fy, cx, cy = intr or intrinsics(cam)
    u, v = _div(fx * x, z) + cx, _div(fy * y, z) + cy               # Camera::Camera2Pixel (src/Camera.cpp:167-171)
    return in_image(cam, u, v, boundary)


def select_local_map(cam, T_cur_w, world: dict, n_local: int = 10, boundary: int = 0, point_capacity: int | None = None) -> dict:
    """Returns kf, kf_dist (n_kf), point, point_kf (min(n_points, point_capacity); None: all), n_close, n_kf, n_points, overflow."""
    Tc = [float(v) for v in np.asarray(T_cur_w, np.float64).reshape(12)]
    P = np.asarray(world["p_world"], np.float64).reshape(-1, 3)
    bad = np.asarray(world["bad"]).reshape(-1)
    Tk = np.asarray(world["T_kf_w"], np.float64).reshape(-1, 12)
    close, intr = [], intrinsics(cam)
    for k, slots in enumerate(world["slots"]):                      # :320
        for p in slots:                                             # :322
            p = int(p)
            if p < 0:                                               # :324
                continue
            X = [float(v) for v in P[p]]
            if X[0] == 0.0 and X[1] == 0.0 and X[2] == 0.0:         # :327 isZero(0)
                continue
            if is_visible(cam, Tc, X, boundary, intr):                    # :330
                dx, dy, dz = Tc[3] - float(Tk[k][3]), Tc[7] - float(Tk[k][7]), Tc[11] - float(Tk[k][11])
                close.append((math.sqrt(dx * dx + (dy * dy + dz * dz)), k))      # :333, Eigen's p0 + (p1 + p2)
                break
    close.sort(key=lambda c: c[0])                                  # :267-268 (stable: equal distances keep map index order)
    chosen = close[:n_local]                                        # :277
    point, point_kf, seen = [], [], set()
    for j, (_, k) in enumerate(chosen):
        for p in world["slots"][k]:
            p = int(p)
            if p < 0 or bad[p] or p in seen:                        # :288, :291, :294
                continue
            seen.add(p)                                             # :297
            point.append(p)
            point_kf.append(j)
    n_points = len(point)
    cap = n_points if point_capacity is None else int(point_capacity)
    return dict(kf=[k for _, k in chosen], kf_dist=[d for d, _ in chosen], point=point[:cap], point_kf=point_kf[:cap],
                n_close=len(close), n_kf=len(chosen), n_points=n_points, overflow=int(n_points > cap))
