"""The restatement of dsdtm_slam_track_commit (include/dsdtm_amd_slam.h, rules T1-T4): a tracked frame's effects on the map — MapPoint::
IncreaseFound for every match of SearchLocalPoints (src/Feature_alignment.cpp:106), the EraseFound walk of Optimizer::PoseOptimization
(src/Optimizer.cpp:81-94) and the SetBadFlag cascade (src/MapPoint.cpp:91-109, :183-198) — in plain numpy over a map image: a world
of track_map_restatement (what DeviceTrackMap.read returns: p_world, bad, found, T_kf_w and per keyframe slots, observes, px, level,
bearing). The yardstick of the device entry and of track_commit_host; it copies nothing from either. Worlds are never changed in
place: every function returns the world after."""
from __future__ import annotations

import numpy as np

MAX_MATCHES, MAX_DESCS = 256, 1024


def copy_world(world) -> dict:
    return {k: ([np.array(a) for a in v] if isinstance(v, list) else np.array(v)) for k, v in world.items()}


def check_desc(world, point, residual_norm):
    """What the entry refuses of one desc (ValueError names it), in the order it checks."""
    point, norm = np.asarray(point, np.int64).reshape(-1), np.asarray(residual_norm, np.float64).reshape(-1)
    if len(point) != len(norm):
        raise ValueError(f"{len(norm)} norms for {len(point)} matches")
    if len(point) > MAX_MATCHES:
        raise ValueError("n_matches out of range")
    if len(point) and (point.min() < 0 or point.max() >= len(world["bad"])):
        raise ValueError("a point index outside the map")
    if len(set(point.tolist())) != len(point):
        raise ValueError("a point occurs twice")
    return point, norm


def track_commit(world, outlier_threshold: float, point, residual_norm):
    """ONE desc, applied wholly. Returns (world after, dict(n_erased, n_bad, bad_points (map indices, in match order), found_after))."""
    if not np.isfinite(outlier_threshold):
        raise ValueError("outlier_threshold is not finite")
    point, norm = check_desc(world, point, residual_norm)
    w = copy_world(world)
    found, bad = w["found"], w["bad"]
    for p in point:                                             # T1: every match, bad or not
        found[p] += 1
    n_erased, went_bad = 0, []
    for p, r in zip(point, norm):                               # T2: behind all of T1, in match order
        if r > outlier_threshold and not bad[p]:                # (strict; a NaN norm compares false)
            found[p] -= 1
            n_erased += 1
            if found[p] <= 0:
                bad[p] = 1
                went_bad.append(int(p))
    for p in went_bad:                                          # T3: the observing slots of a point that went bad here, in every keyframe
        for slots, observes in zip(w["slots"], w["observes"]):
            hit = (slots == p) & (observes != 0)
            slots[hit] = -1
            observes[hit] = 0
    return w, dict(n_erased=n_erased, n_bad=len(went_bad), bad_points=went_bad, found_after=[int(found[p]) for p in point])


KF_MAX_POINTS, KF_MAX_LOCAL_KF = 4096, 64


def camera_centre(T12):
    """Get_CameraCnt from [R|t]: c_i = -((R_0i t_0 + R_1i t_1) + R_2i t_2), separate multiplies and adds in this order."""
    T = [float(v) for v in np.asarray(T12, np.float64).reshape(12)]
    return [-((T[c] * T[3] + T[4 + c] * T[7]) + T[8 + c] * T[11]) for c in range(3)]


def gather_keyframe_desc(world, T_cur_w, n_valid: int, cur_point, kf: int, local_kf) -> dict:
    """The gather of dsdtm_slam_need_keyframes: one tracker's inputs of dsdtm_need_keyframes (the dict capi.KeyframeCall and
    keyframe_decision take) from a map image and indices. The last keyframe's list is its slots in slot order with point_of_slot >= 0,
    observing or not. ValueError names what the entry refuses."""
    T = np.asarray(T_cur_w, np.float64).reshape(12)
    cur, lk = np.asarray(cur_point, np.int64).reshape(-1), np.asarray(local_kf, np.int64).reshape(-1)
    P, K = len(world["bad"]), len(world["slots"])
    if len(cur) > KF_MAX_POINTS:
        raise ValueError("n_cur_points out of range")
    if len(lk) > KF_MAX_LOCAL_KF:
        raise ValueError("n_local_kf out of range")
    if not 0 <= kf < K:
        raise ValueError("kf is not a keyframe of the map")
    if not np.all(np.isfinite(T)):
        raise ValueError("T_cur_w is not finite")
    if len(cur) and (cur.min() < 0 or cur.max() >= P):
        raise ValueError("cur_point outside the map")
    if len(lk) and (lk.min() < 0 or lk.max() >= K):
        raise ValueError("local_kf outside the map")
    listed = np.asarray([p for p in world["slots"][kf] if p >= 0], np.int64)
    pw, bad = np.asarray(world["p_world"], np.float64).reshape(-1, 3), np.asarray(world["bad"], np.uint8)
    return dict(T_cur_w=T.copy(), T_kf_w=np.asarray(world["T_kf_w"][kf], np.float64).reshape(12).copy(), n_valid=int(n_valid),
                cur_p_world=pw[cur].reshape(-1, 3).copy(), cur_bad=bad[cur].copy(), kf_p_world=pw[listed].reshape(-1, 3).copy(), kf_bad=bad[listed].copy(),
                local_kf_centre=np.array([camera_centre(world["T_kf_w"][k]) for k in lk], np.float64).reshape(-1, 3))


def track_commit_call(worlds, outlier_threshold: float, descs, bad_capacity: int | None = None):
    """One call: `descs` is a list of (world index, point, residual_norm), applied in desc order (T4: descs on one map each wholly
    before the next; descs on different maps never meet). Every desc is checked before any is applied. Returns (worlds after, one
    result dict per desc; with bad_capacity also overflow_bad, and bad_points cut to it)."""
    if len(descs) > MAX_DESCS:
        raise ValueError("n out of range")
    if not np.isfinite(outlier_threshold):
        raise ValueError("outlier_threshold is not finite")
    if bad_capacity is not None and bad_capacity < 0:
        raise ValueError("bad_capacity is negative")
    for m, point, norm in descs:
        check_desc(worlds[m], point, norm)
    now, results = list(worlds), []
    for m, point, norm in descs:
        now[m], r = track_commit(now[m], outlier_threshold, point, norm)
        if bad_capacity is not None:
            r["overflow_bad"] = int(r["n_bad"] > bad_capacity)
            r["bad_points"] = r["bad_points"][:bad_capacity]
        results.append(r)
    return now, results
