"""Tracking::CraeteKeyframe (reference src/Tracking.cpp:412-464) from the per-cell corners on, restated once in plain Python / numpy,
line by line — the yardstick the device entry (dsdtm_newkf_make, csrc/newkf.hip) and the host function (create_keyframe_host,
host/dsdtm_newkf_host.hpp) are held to. No device, no library call. The rules K1-K6 are those of include/dsdtm_amd_newkf.h.

Routines it follows: Feature_detector::detect behind the image work (src/Feature_detection.cpp:110-153), Frame::Set_Mask
(src/Frame.cpp:286-298) with cv::circle(.., -1) as OpenCV's drawing.cpp Circle() fills it, Frame::Add_Feature's bearing
(src/Frame.cpp:139-149), Frame::Get_FeatureDetph(cv::Point2f) and Frame::UnProject (src/Frame.cpp:152-157, 201-224),
Camera::Pixel2Camera(cv::Point2f, float) (src/Camera.cpp:173-178).

The mask is a REAL image here, painted row by row as the reference paints it; nothing is shared with the half-width table the device
and the host function test against. Float arithmetic is numpy float32 scalar by scalar, double arithmetic Python floats: every
product and sum rounds on its own (no fused multiply-add).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32


@dataclass
class NewKeyframeParams:
    """dsdtm_newkf_params"""
    width: int
    height: int
    cell_size: int
    grid_cols: int
    grid_rows: int
    max_fts: int
    min_dist: int
    score_floor: float = 20.0      # the literal of src/Feature_detection.cpp:128


@dataclass
class NewKeyframeInput:
    """One tracker: dsdtm_newkf_desc without the capacities."""
    cell_score: np.ndarray          # G float32
    cell_x: np.ndarray              # G int32
    cell_y: np.ndarray
    cell_level: np.ndarray
    depth: np.ndarray               # height x width uint16
    depth_scale: float
    T_c2w: np.ndarray               # 12 doubles
    first_point_index: int = 0
    px_xy: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.float32))
    level: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    bearing: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.float64))
    has_point: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint8))
    initial: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint8))
    point_index: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    dyn_mask: np.ndarray | None = None      # height x width uint8

    @property
    def n_existing(self) -> int:
        return int(np.asarray(self.px_xy).reshape(-1, 2).shape[0])


COLUMNS = ("point_of_slot", "observes", "px_xy", "level", "bearing", "depth_of_slot", "new_p_world")


def cv_round(v) -> int:
    """cvRound of a value narrowed to float: to nearest, halves to even."""
    return int(np.rint(F32(v)))


def paint_circle(mask: np.ndarray, cx: int, cy: int, radius: int):
    """cv::circle(mask, (cx, cy), radius, 0, -1): OpenCV drawing.cpp Circle() with fill — the midpoint walk, two pairs of rows per step,
    each row clipped to the image."""
    h, w = mask.shape

    def row(y, x1, x2):
        if 0 <= y < h:
            x1, x2 = max(x1, 0), min(x2, w - 1)
            if x1 <= x2:
                mask[y, x1:x2 + 1] = 0
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        row(cy - dy, cx - dx, cx + dx)
        row(cy + dy, cx - dx, cx + dx)
        row(cy - dx, cx - dy, cx + dy)
        row(cy + dx, cx - dy, cx + dy)
        dy += 1
        err += plus
        plus += 2
        m = 0 if err <= 0 else -1
        err -= minus & m
        dx += m
        minus -= m & 2


def walk(prm: NewKeyframeParams, inp: NewKeyframeInput) -> list:
    """K1-K4: the (x, y, level) of the features detect() adds, in the order it adds them."""
    n = inp.n_existing
    if n >= prm.max_fts:                                                   # K1 (:71-72)
        return []
    score = np.asarray(inp.cell_score, np.float32)
    # K2 (:110): descending score, equal scores in cell order; a NaN never passes score > floor and is dropped first
    cand = [k for k in range(prm.grid_cols * prm.grid_rows) if float(score[k]) > float(F32(prm.score_floor))]
    cand.sort(key=lambda k: -float(score[k]))                              # (stable)
    mask = np.full((prm.height, prm.width), 255, np.uint8)                # src/Frame.cpp:64
    if n > 0:                                                              # K3 (:119-122): Set_Mask only on a frame that has features
        px = np.asarray(inp.px_xy, np.float32).reshape(-1, 2)
        for k in range(n):
            if inp.has_point[k]:
                paint_circle(mask, cv_round(px[k, 0]), cv_round(px[k, 1]), prm.min_dist)
        if inp.dyn_mask is not None:                                       # threshold at 200, then the saturating subtraction
            mask[np.asarray(inp.dyn_mask, np.uint8) > 200] = 0
    out = []
    for k in cand:                                                         # K4 (:124-150)
        x, y, lvl = int(inp.cell_x[k]), int(inp.cell_y[k]), int(inp.cell_level[k])
        if not (0 <= x < prm.width and 0 <= y < prm.height) or not 0 <= lvl <= 15:
            continue                                                       # (the reference indexes the cv::Mat unchecked)
        if mask[y, x] != 255:
            continue
        out.append((x, y, lvl))
        paint_circle(mask, x, y, prm.cell_size)
        n += 1
        if n >= prm.max_fts:
            break
    return out


def feature_depth(depth: np.ndarray, inv_scale, px, py) -> np.float32:
    """Frame::Get_FeatureDetph(cv::Point2f) on the u16 image kept as d * (1.0f / depth_scale); -1 where there is none."""
    h, w = depth.shape
    x, y = cv_round(px), cv_round(py)
    if not (0 <= x < w and 0 <= y < h):
        return F32(-1.0)
    d = F32(depth[y, x]) * inv_scale
    if d != 0:
        return d
    for ddx, ddy in ((-1, 0), (0, -1), (1, 0), (0, 1)):
        xx, yy = x + ddx, y + ddy
        if 0 <= xx < w and 0 <= yy < h:
            d = F32(depth[yy, xx]) * inv_scale
            if d != 0:
                return d
    return F32(-1.0)


def bearing_of(cam, px, py):
    """Frame::Add_Feature: Pixel2Camera(cv::Point2f, 1.0f) in float, normalised in double."""
    fx, fy, cx, cy = (F32(v) for v in cam)
    one = F32(1.0)
    bx, by = float((one * (F32(px) - cx)) / fx), float((one * (F32(py) - cy)) / fy)
    n = math.sqrt(bx * bx + by * by + 1.0 * 1.0)
    return (bx / n, by / n, 1.0 / n)


def unproject(cam, T, px, py, d):
    """Frame::UnProject: Pixel2Camera in float, then mT_c2w.inverse() * p as Sophus evaluates it: R^T p + (-(R^T t))."""
    fx, fy, cx, cy = (F32(v) for v in cam)
    p0, p1, p2 = float(d * (F32(px) - cx) / fx), float(d * (F32(py) - cy) / fy), float(d)
    T = [float(v) for v in np.asarray(T, np.float64).reshape(12)]
    out = []
    for c in range(3):
        rp = T[c] * p0 + T[4 + c] * p1 + T[8 + c] * p2
        rt = T[c] * T[3] + T[4 + c] * T[7] + T[8 + c] * T[11]
        out.append(rp + (-rt))
    return out


def create_keyframe(cam, prm: NewKeyframeParams, inp: NewKeyframeInput) -> dict:
    """K1-K6. cam = (fx, fy, cx, cy). Returns n_new, n_slots, n_new_points and the COLUMNS of dsdtm_newkf_result."""
    new = walk(prm, inp)
    ne, n_slots = inp.n_existing, inp.n_existing + len(new)
    px = np.zeros((n_slots, 2), np.float32)
    level = np.zeros(n_slots, np.int32)
    bearing = np.zeros((n_slots, 3), np.float64)
    px[:ne] = np.asarray(inp.px_xy, np.float32).reshape(-1, 2)
    level[:ne] = inp.level
    bearing[:ne] = np.asarray(inp.bearing, np.float64).reshape(-1, 3)
    for j, (x, y, lvl) in enumerate(new):                                  # K5 (:145)
        px[ne + j] = (x, y)
        level[ne + j] = lvl
        bearing[ne + j] = bearing_of(cam, px[ne + j, 0], px[ne + j, 1])
    point_of_slot = np.full(n_slots, -1, np.int32)
    observes = np.zeros(n_slots, np.uint8)
    depth_of_slot = np.full(n_slots, -1.0, np.float32)
    points = []
    inv = F32(1.0) / F32(inp.depth_scale)
    depth = np.asarray(inp.depth, np.uint16)
    for i in range(n_slots):                                               # K6 (src/Tracking.cpp:424-455)
        if i < ne and inp.initial[i]:
            point_of_slot[i], observes[i] = int(inp.point_index[i]), 1
            continue
        z = feature_depth(depth, inv, px[i, 0], px[i, 1])
        depth_of_slot[i] = z
        if z < 0:
            continue
        point_of_slot[i], observes[i] = inp.first_point_index + len(points), 1
        points.append(unproject(cam, inp.T_c2w, px[i, 0], px[i, 1], z))
    return {"n_new": len(new), "n_slots": n_slots, "n_new_points": len(points), "point_of_slot": point_of_slot, "observes": observes,
            "px_xy": px, "level": level, "bearing": bearing, "depth_of_slot": depth_of_slot,
            "new_p_world": np.asarray(points, np.float64).reshape(-1, 3)}
