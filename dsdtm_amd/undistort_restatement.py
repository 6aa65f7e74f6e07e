"""The rules U1-U5 of include/dsdtm_amd_undistort.h restated in numpy: THE YARDSTICK of libdsdtm_amd_undistort.so and of the host functions
of dsdtm_amd/host/dsdtm_undistort_host.hpp, which are bit-equal to it. U1 and U5 are float64 with one numpy operation per rounding, in the
header's order (numpy never fuses a multiply with an add); U2 and U3 are integers. The OpenCV calls whose documented shape this keeps
(cv::undistort = initUndistortRectifyMap + remap at INTER_BITS = 5, cv::undistortPoints with P = K) are not available to this project;
parity with OpenCV's fixed-point remap is unpinned. Nothing of the product imports this module. (`rounding` of undistort_map and `bias` of
remap_gray are the hooks through which tests/undistort_cases.py builds its two deliberately wrong variants.)"""
from __future__ import annotations

import numpy as np

OUTSIDE = -2**31           # DSDTM_UNDISTORT_OUTSIDE
MIN_SIDE, MAX_SIDE, MAX_FRAMES, MAX_POINTS = 8, 4096, 1024, 16384
ITERATIONS = 5             # cv::undistortPoints of OpenCV 2.4: a fixed count


def model(cam, dist):
    """(fx, fy, cx, cy) and (k1, k2, p1, p2, k3): float32 values widened to float64, as mInstrinsicMat (CV_32F) is read."""
    K = [np.float64(np.float32(v)) for v in cam[:4]]
    D = [np.float64(np.float32(v)) for v in dist]
    return K, D


def _terms(D, x, y):
    """den = 1 + ((k3 r2 + k2) r2 + k1) r2, dx, dy: the terms U1 and U5 share, one rounding per operation."""
    k1, k2, p1, p2, k3 = D
    r2 = x * x + y * y
    den = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    dx = ((2.0 * p1) * x) * y + p2 * (r2 + (2.0 * x) * x)
    dy = p1 * (r2 + (2.0 * y) * y) + ((2.0 * p2) * x) * y
    return den, dx, dy


def cv_round_sat(v):
    """cvRound (halves to even) saturated to int32; not finite: OUTSIDE."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.clip(np.where(np.isfinite(v), v, 0.0), -2147483648.0, 2147483647.0)).astype(np.int64)
    return np.where(np.isfinite(v), r, OUTSIDE).astype(np.int32)


def forward(cam, dist, x, y):
    """U1 steps 2-6 on normalised coordinates: the distorted PIXEL (mx, my) of the ideal point (x, y)."""
    (fx, fy, cx, cy), D = model(cam, dist)
    with np.errstate(all="ignore"):
        radial, dx, dy = _terms(D, x, y)
        xd = x * radial + dx
        yd = y * radial + dy
        return xd * fx + cx, yd * fy + cy


def undistort_map(cam, dist, width, height, rounding=cv_round_sat):
    """U1: (height, width, 2) int32, the pairs (X, Y) at 1/32 pixel."""
    (fx, fy, cx, cy), _ = model(cam, dist)
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    with np.errstate(all="ignore"):
        mx, my = forward(cam, dist, (u - cx) / fx, (v - cy) / fy)
        return np.stack([rounding(mx * 32.0), rounding(my * 32.0)], axis=-1)


def _tap(src, x, y):
    h, w = src.shape
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    return np.where(inside, src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0).astype(np.int64), inside


def remap_gray(m, src, bias=512):
    """U2: integer bilinear with borders 0. src: (height, width) uint8 of the map's size."""
    X, Y = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    x0, ax, y0, ay = X >> 5, X & 31, Y >> 5, Y & 31
    p00, p01, p10, p11 = (_tap(src, x0 + i, y0 + j)[0] for j in (0, 1) for i in (0, 1))
    return (((32 - ax) * (32 - ay) * p00 + ax * (32 - ay) * p01 + (32 - ax) * ay * p10 + ax * ay * p11 + bias) >> 10).astype(np.uint8)


def taps_outside(m, width, height):
    """How many of the four taps of U2 lie outside the source, per destination pixel (0..4)."""
    X, Y = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    probe = np.zeros((height, width), np.uint8)
    return 4 - sum(_tap(probe, (X >> 5) + i, (Y >> 5) + j)[1].astype(np.int64) for j in (0, 1) for i in (0, 1))


def remap_depth(m, src):
    """U3: nearest neighbour, outside 0. src: (height, width) uint16."""
    X, Y = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    return _tap(src, (X + 16) >> 5, (Y + 16) >> 5)[0].astype(np.uint16)


def undistort_frame(m, gray, depth=None):
    """One frame of U4: (gray', depth' or None)."""
    return remap_gray(m, gray), (remap_depth(m, depth) if depth is not None else None)


def bearing(cam, px):
    """Frame::Add_Feature's rule (include/dsdtm_amd_newkf.h K5): Pixel2Camera(px, 1.0f) in float, normalised in double."""
    fx, fy, cx, cy = (np.float32(v) for v in cam[:4])
    px = np.asarray(px, np.float32).reshape(-1, 2)
    one = np.float32(1.0)
    bx = ((one * (px[:, 0] - cx)) / fx).astype(np.float64)
    by = ((one * (px[:, 1] - cy)) / fy).astype(np.float64)
    nrm = np.sqrt(bx * bx + by * by + 1.0 * 1.0)
    return np.stack([bx / nrm, by / nrm, 1.0 / nrm], axis=1)


def undistort_points(cam, dist, px_in, skip=None, px_out=None, bearing_out=None, iterations=ITERATIONS):
    """U5: (px_out (n, 2) float32, bearing_out (n, 3) float64); rows of bearing_out where skip != 0 keep what they held (zeros if none given)."""
    (fx, fy, cx, cy), D = model(cam, dist)
    px_in = np.asarray(px_in, np.float32).reshape(-1, 2)
    n = len(px_in)
    skip = np.zeros(n, np.uint8) if skip is None else np.asarray(skip, np.uint8)
    out = np.empty((n, 2), np.float32) if px_out is None else px_out
    b = np.zeros((n, 3), np.float64) if bearing_out is None else bearing_out
    x0 = (px_in[:, 0].astype(np.float64) - cx) / fx
    y0 = (px_in[:, 1].astype(np.float64) - cy) / fy
    x, y = x0, y0
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            den, dx, dy = _terms(D, x, y)
            icdist = 1.0 / den
            x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
        und = np.stack([(x * fx + cx).astype(np.float32), (y * fy + cy).astype(np.float32)], axis=1)
        keep = skip != 0
        new_b = bearing(cam, und)
    out[:] = np.where(keep[:, None], px_in, und)
    b[~keep] = new_b[~keep]
    return out, b
