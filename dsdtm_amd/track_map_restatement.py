"""dsdtm_trackmap_local (include/dsdtm_amd_trackmap.h) restated in numpy: local_map_restatement.select_local_map plus the flatten
definition — the yardstick the device entry (csrc/trackmap.hip) and the host function (flatten_local_map_host,
host/dsdtm_trackmap_host.hpp) are held to. No device, no library call.

A world is the selection's map (p_world, bad, T_kf_w, slots: local_map_restatement) plus found (P, int32) and, per keyframe, observes
(0 / 1 per slot), px (n_slots x 2 float32), level (n_slots int32) and bearing (n_slots x 3 float64). Nothing here computes with a
float: every column is a copy.
"""
from __future__ import annotations

import numpy as np

from . import local_map_restatement as R

MAX_LOCAL_POINTS = 4096


def flatten(world: dict, points, obs_capacity: int | None = None) -> dict:
    """The columns for the emitted `points` (map indices, in list order). Point i's observations are the observing slots
    (observes == 1, point_of_slot == the point) of ALL keyframes in ascending (keyframe, slot) order — two observing slots of one
    keyframe on one point (the caller's violated duty) are two observations. off is the full prefix sum and n_obs its end; the
    observation columns hold the first min(n_obs, obs_capacity) (None: all)."""
    points = [int(p) for p in points]
    P = np.asarray(world["p_world"], np.float64).reshape(-1, 3)
    m = len(points)
    per_point = {p: [] for p in points}
    for k, (slots, obs) in enumerate(zip(world["slots"], world["observes"])):          # ascending keyframe ...
        for s in np.flatnonzero(np.asarray(obs) != 0):                                  # ... and slot
            p = int(slots[s])
            if p in per_point:
                per_point[p].append((k, int(s)))
    off = np.zeros(m + 1, np.int32)
    pairs = []
    for i, p in enumerate(points):
        pairs += per_point[p]
        off[i + 1] = len(pairs)
    n_obs = len(pairs)
    pairs = pairs[:n_obs if obs_capacity is None else int(obs_capacity)]
    n = len(pairs)
    okf = np.array([k for k, _ in pairs], np.int32).reshape(n)
    opx, olv, ob = np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.zeros((n, 3), np.float64)
    for j, (k, s) in enumerate(pairs):
        opx[j], olv[j], ob[j] = world["px"][k][s], world["level"][k][s], world["bearing"][k][s]
    return dict(pw=P[points].reshape(m, 3).copy(), found=np.asarray(world["found"], np.int32)[points].reshape(m).copy(),
                bad=np.asarray(world["bad"], np.uint8)[points].reshape(m).copy(), off=off, okf=okf, opx=opx, olv=olv, ob=ob, n_obs=n_obs)


def track_map_local(cam, T_cur_w, world: dict, n_local: int = 10, boundary: int = 0, point_capacity: int = MAX_LOCAL_POINTS,
                    obs_capacity: int | None = None) -> dict:
    """The selection's answer (kf, kf_dist, point, point_kf, n_close, n_kf, n_points), overflow_points / overflow_obs, n_obs and
    `flat`: the columns with the keys of tracking.flatten_local_map."""
    sel = R.select_local_map(cam, T_cur_w, world, n_local, boundary, point_capacity)
    flat = flatten(world, sel["point"], obs_capacity)
    n_obs = flat.pop("n_obs")
    out = {k: sel[k] for k in ("kf", "kf_dist", "point", "point_kf", "n_close", "n_kf", "n_points")}
    out.update(overflow_points=sel["overflow"], n_obs=n_obs, overflow_obs=int(obs_capacity is not None and n_obs > int(obs_capacity)), flat=flat)
    return out
