"""The three entries of include/dsdtm_amd_mapping.h restated in plain Python over a WORLD (track_map_restatement's: p_world, bad, found,
T_kf_w and per keyframe slots, observes, px, level, bearing): the yardstick of libdsdtm_amd_mapping.so and of
host/dsdtm_mapping_host.hpp. Written from the reference's sources, statement by statement, with this project's one definition where
the reference iterates by pointer value: a std::map<KeyFrame*, ...> is walked in ascending keyframe index.

    update_connection   KeyFrame::UpdateConnection               src/Keyframe.cpp:71-133
    ba_window           Optimizer::LocalBundleAdjustment         src/Optimizer.cpp:109-159 (the sets), :166-224 (the blocks)
    ba_commit           the write-back and the outlier pass      src/Optimizer.cpp:236-271, MapPoint::Erase_Observation / SetBadFlag
                                                                 src/MapPoint.cpp:57-109

No floating-point operation happens anywhere: every value is a copy. mapping.MapPoint.SetBadFlag only sets a flag; the rule the commit
needs (SetBadFlag clears mObservations and erases the match in every observer) is restated here.
"""
from __future__ import annotations

import copy

import numpy as np

COV_THRESHOLD = 15
MAX_PAIRS, MAX_WINDOWS, MAX_COV = 1024, 256, 255
MAX_FREE_KF, MAX_CONST_KF, MAX_POINTS, MAX_OBSERVATIONS = 16, 64, 16384, 131072
FLAGS = ("over_free_kf", "over_const_kf", "over_points", "over_obs", "over_keyframe_capacity", "over_point_capacity", "over_observation_capacity")


def observations(world) -> dict:
    """mObservations of every point: point -> [(keyframe, slot)], ascending. A slot is an observation when it observes."""
    obs = {}
    for k, (slots, flags) in enumerate(zip(world["slots"], world["observes"])):
        for s in np.flatnonzero(np.asarray(flags) == 1):
            obs.setdefault(int(slots[s]), []).append((k, int(s)))
    return obs


def update_connection(world, kf: int, capacity: int | None = None) -> dict:
    obs = observations(world)
    weight = {}                                             # tKFLocalMap
    for p in world["slots"][kf]:                            # :78-96: mvMapPoints is walked; the slot's own flag is not consulted
        p = int(p)
        if p < 0 or world["bad"][p]:
            continue
        for k, _ in obs.get(p, ()):
            if k != kf:
                weight[k] = weight.get(k, 0) + 1
    pairs = []
    if weight:                                              # :98-99
        best_w, best_k = 0, None
        for k in sorted(weight):                            # :107-120
            if weight[k] > best_w:
                best_w, best_k = weight[k], k
            if weight[k] > COV_THRESHOLD:
                pairs.append((weight[k], k))
        if not pairs:
            pairs.append((best_w, best_k))
        pairs.sort()                                        # :129
    cap = len(pairs) if capacity is None else capacity
    return dict(n_cov=len(pairs), n_connected=len(weight), overflow=int(len(pairs) > cap), cov_kf=[k for _, k in pairs[:cap]],
                cov_weight=[w for w, _ in pairs[:cap]])


def ba_window(world, kf: int, cov_kf, origin_kf: int = -1, keyframe_capacity: int | None = None, point_capacity: int | None = None,
              observation_capacity: int | None = None) -> dict:
    """The window the reference builds the first time it is asked for `kf`. Returns the result's fields and, when usable, the
    problem's columns with the three index arrays."""
    obs = observations(world)
    local = [kf] + [int(k) for k in cov_kf]                 # W1 :110-121
    points, listed = [], set()
    for k in local:                                         # W2 :123-141
        for p in world["slots"][k]:
            p = int(p)
            if p < 0 or world["bad"][p]:
                continue
            if kf == origin_kf:                             # mlLocalBAKFId starts at 0 = tKFrame->mlId: :135 fails for every point
                continue
            if p not in listed:
                listed.add(p)
                points.append(p)
    fixed = []
    for p in points:                                        # W3 :143-159
        for k, _ in obs.get(p, ()):
            if k not in local and k not in fixed:
                fixed.append(k)
    n_obs = sum(len(obs.get(p, ())) for p in points)
    origin_local = int(origin_kf in local)
    r = dict(n_local=len(local), n_fixed=len(fixed), n_points=len(points), n_obs=n_obs)
    kcap = len(local) + len(fixed) if keyframe_capacity is None else keyframe_capacity
    pcap = len(points) if point_capacity is None else point_capacity
    ocap = n_obs if observation_capacity is None else observation_capacity
    n_free = len(local) - origin_local
    r.update(over_free_kf=int(n_free > MAX_FREE_KF), over_const_kf=int(len(fixed) + origin_local > MAX_CONST_KF), over_points=int(len(points) > MAX_POINTS),
             over_obs=int(n_obs > MAX_OBSERVATIONS), over_keyframe_capacity=int(len(local) + len(fixed) > kcap), over_point_capacity=int(len(points) > pcap),
             over_observation_capacity=int(n_obs > ocap))
    r["usable"] = int(n_free >= 1 and not any(r[f] for f in FLAGS))
    if not r["usable"]:
        return r
    window_kf = local + fixed
    at = {k: i for i, k in enumerate(window_kf)}
    okf, opt, oslot, obear, olevel = [], [], [], [], []
    for i, p in enumerate(points):                          # W4 :202-224
        for k, s in obs.get(p, ()):
            okf.append(at[k]); opt.append(i); oslot.append((k << 32) | s)
            obear.append(world["bearing"][k][s]); olevel.append(world["level"][k][s])
    r.update(kf_index=np.array(window_kf, np.int32), kf_constant=np.array([int(k == origin_kf) for k in local] + [1] * len(fixed), np.uint8),
             T_c2w=np.array([world["T_kf_w"][k] for k in window_kf], np.float64).reshape(-1, 12), point_index=np.array(points, np.int32),
             points=np.array([world["p_world"][p] for p in points], np.float64).reshape(-1, 3), obs_kf=np.array(okf, np.int32),
             obs_point=np.array(opt, np.int32), obs_slot=np.array(oslot, np.int64), obs_bearing=np.array(obear, np.float64).reshape(-1, 3),
             obs_level=np.array(olevel, np.int32))
    return r


def overlap(windows) -> tuple | None:
    """The smallest (first, second) pair of usable windows that share a keyframe or a point of one map; windows: [(map id, window)]."""
    best = None
    for b, (mb, wb) in enumerate(windows):
        for a, (ma, wa) in enumerate(windows[:b]):
            if ma != mb or not wa["usable"] or not wb["usable"]:
                continue
            if set(wa["kf_index"].tolist()) & set(wb["kf_index"].tolist()) or set(wa["point_index"].tolist()) & set(wb["point_index"].tolist()):
                best = min(best, (a, b)) if best else (a, b)
    return best


def ba_commit(world, window, T_c2w, points, outlier, bad_capacity: int | None = None):
    """One usable window with the solver's poses, points and outlier flags: (the world afterwards — a copy —, the result)."""
    w = copy.deepcopy(world)
    for i, k in enumerate(window["kf_index"]):              # C1 :237-242
        w["T_kf_w"][k] = np.asarray(T_c2w, np.float64).reshape(-1, 12)[i]
    for i, p in enumerate(window["point_index"]):           # :244-248
        w["p_world"][p] = np.asarray(points, np.float64).reshape(-1, 3)[i]
    n_outliers, bad = 0, []
    for i, p in enumerate(window["point_index"]):           # C2 :255-272
        p = int(p)
        mine = [j for j in range(len(window["obs_point"])) if window["obs_point"][j] == i]
        m_obs = {int(window["obs_slot"][j]) >> 32: int(window["obs_slot"][j]) & 0xffffffff for j in mine}      # mObservations
        m_obs_num = len(mine)                               # mObsNum (the caller's duty: one observing slot per keyframe)
        for j in mine:                                      # tMpObserves is a COPY: the walk goes on after the point went bad
            if not outlier[j]:
                continue
            n_outliers += 1
            k, s = int(window["obs_slot"][j]) >> 32, int(window["obs_slot"][j]) & 0xffffffff
            if k in m_obs:                                  # Erase_Observation src/MapPoint.cpp:57-82
                m_obs_num -= 1
                del m_obs[k]
                w["observes"][k][s] = 0
                if m_obs_num <= 1:                          # SetBadFlag :91-109
                    for k2, s2 in m_obs.items():
                        w["observes"][k2][s2] = 0
                        w["slots"][k2][s2] = -1             # Erase_MapPointMatch(index)
                    m_obs.clear()
                    w["bad"][p] = 1
                    bad.append(p)
            # Erase_MapPointMatch(MapPoint*) :267 asks the point for its index in the keyframe, finds none, and leaves mvMapPoints alone
    cap = len(bad) if bad_capacity is None else bad_capacity
    return w, dict(n_outliers=n_outliers, n_bad=len(bad), overflow_bad=int(len(bad) > cap), bad_points=bad[:cap])
