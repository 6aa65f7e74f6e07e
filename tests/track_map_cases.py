"""The worlds of dsdtm_trackmap_local (include/dsdtm_amd_trackmap.h), shared by the CPU and the GPU half of the tests: small maps built
deterministically from mapping.py objects — KeyFrame / MapPoint with the reference's observation bookkeeping, extended by what
tracking.flatten_local_map reads (mObservations by keyframe index, Get_FoundNums, the keyframe's px / level / bearing columns), so that
tracking.flatten_local_map is the yardstick of the flatten. A case is a dict: name, kfs, mps (the objects; None where arrays were
edited by hand), world (track_map_restatement's), poses, n_local, point_capacity, obs_capacity (None: room for all). expected(case) is the
restatement's answer per pose, computed once per session. Test infrastructure only."""
import struct

import numpy as np

from dsdtm_amd import mapping
from dsdtm_amd import track_map_restatement as TR
from tests.local_map_cases import CAM, I12, at_pixel, pose

FLAT_KEYS = ("pw", "found", "bad", "off", "okf", "opx", "olv", "ob")
BITS = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}


class Feature(mapping.Feature):
    def __init__(self, normal, level, mpx):
        super().__init__(normal, level)
        self.mpx = np.asarray(mpx, np.float32)


class KeyFrame(mapping.KeyFrame):
    """mapping.KeyFrame + its features' columns as flatten_local_map reads them (mvFeatures of a keyframe does not change)."""

    def __init__(self, mlId, T, features):
        super().__init__(mlId, T, features, mapping.Camera(512.0))
        n = len(features)
        self.px = np.array([f.mpx for f in features], np.float32).reshape(n, 2)
        self.level = np.array([f.mlevel for f in features], np.int32)
        self.bearing = np.array([f.mNormal for f in features], np.float64).reshape(n, 3)


class MapPoint(mapping.MapPoint):
    """mapping.MapPoint + the found counter and mObservations keyed by the keyframe's index (its mlId: keyframes are numbered in the
    order they are added)."""
    mnFound = 1

    def Get_FoundNums(self):
        return self.mnFound

    @property
    def mObservations(self):
        return {kf.mlId: idx for kf, idx in self._obs.items()}


def world_of(kfs, mps):
    """The objects as a world of the restatement. A slot observes when its point's mObservations holds (this keyframe, this slot)."""
    index = {id(mp): i for i, mp in enumerate(mps)}
    slots = [np.array([-1 if mp is None else index[id(mp)] for mp in kf.mvMapPoints], np.int32) for kf in kfs]
    observes = [np.array([0 if mp is None else int(mp.Get_IndexInKeyFrame(kf) == s) for s, mp in enumerate(kf.mvMapPoints)], np.uint8) for kf in kfs]
    return dict(p_world=np.array([mp.Get_Pose() for mp in mps], np.float64).reshape(-1, 3), bad=np.array([int(mp.IsBad()) for mp in mps], np.uint8),
                found=np.array([mp.Get_FoundNums() for mp in mps], np.int32),
                T_kf_w=np.array([kf.Get_Pose().reshape(12) for kf in kfs], np.float64).reshape(-1, 12), slots=slots, observes=observes,
                px=[kf.px for kf in kfs], level=[kf.level for kf in kfs], bearing=[kf.bearing for kf in kfs])


class Builder:
    def __init__(self, seed=1, step=0.1):
        self.rng, self.step, self.kfs, self.mps = np.random.default_rng(seed), step, [], []

    def keyframe(self, n_slots, x=None):
        """A keyframe at camera centre (x, 0, 0) (default: step * its index) looking along +z, every slot NULL."""
        k = len(self.kfs)
        x = self.step * k if x is None else x
        feats = []
        for _ in range(n_slots):
            nrm = self.rng.normal(size=3)
            feats.append(Feature(nrm / np.linalg.norm(nrm), int(self.rng.integers(0, 4)), self.rng.uniform((1, 1), (638, 478))))
        kf = KeyFrame(k, np.array(pose((-x, 0.0, 0.0))).reshape(3, 4), feats)
        kf.centre_x = x
        self.kfs.append(kf)
        return kf

    def new_point(self, kf, s, observe=True):
        """A new map point where slot s of kf sees it (so the keyframe's own pose projects it into the image)."""
        X = np.array(at_pixel(float(kf.px[s][0]), float(kf.px[s][1]), float(self.rng.uniform(2.0, 4.0)))) + (kf.centre_x, 0.0, 0.0)
        mp = MapPoint(len(self.mps), X)
        mp.mnFound = int(self.rng.integers(1, 60))
        self.mps.append(mp)
        self.link(kf, s, mp, observe)
        return mp

    @staticmethod
    def link(kf, s, mp, observe=True):
        kf.Add_MapPoint(mp, s)
        if observe:
            mp.Add_Observation(kf, s)

    def trajectory(self, n_kf, n_slots, share=0.4, null=0.1, back=3):
        """Keyframes along x; a slot is NULL, re-observes a point of the last `back` keyframes, or makes a new point."""
        for _ in range(n_kf):
            kf = self.keyframe(n_slots)
            lo = max(0, len(self.mps) - back * n_slots)
            for s in range(n_slots):
                r = self.rng.random()
                if r < null:
                    continue
                if r < null + share and len(self.mps) > lo:
                    mp = self.mps[int(self.rng.integers(lo, len(self.mps)))]
                    if mp.Get_IndexInKeyFrame(kf) < 0 and mp not in kf.mvMapPoints:
                        self.link(kf, s, mp)
                        continue
                self.new_point(kf, s)
        return self


def case(name, b, poses, n_local=10, point_capacity=TR.MAX_LOCAL_POINTS, obs_capacity=None, **extra):
    return dict(name=name, kfs=b.kfs, mps=b.mps, world=world_of(b.kfs, b.mps), poses=[list(p) for p in poses], n_local=n_local, boundary=0,
                point_capacity=point_capacity, obs_capacity=obs_capacity, **extra)


def plain():                                                 # a)
    b = Builder(1).trajectory(12, 24)
    return case("plain_trajectory", b, [pose((-0.32, 0, 0)), pose((-0.9, 0.01, 0.02), yaw=0.03)], n_local=4)


def outside_observers():                                     # b)
    b = Builder(2).trajectory(12, 16)
    last = b.keyframe(8, x=9.0)                               # far away: never local, the highest index
    for s, mp in enumerate([mp for mp in b.kfs[0].mvMapPoints if mp is not None][:5]):
        b.link(last, s, mp)
    return case("observed_from_outside_the_local_set", b, [pose((-0.02, 0, 0))], n_local=2)


def ba_quirk():                                              # c)
    b = Builder(3)
    kfs = [b.keyframe(8) for _ in range(4)]
    mp = b.new_point(kfs[0], 2)
    for kf in kfs[1:]:
        b.link(kf, 5, mp)
    for kf in kfs:
        for s in (0, 1):
            b.new_point(kf, s)
    mp.Erase_Observation(kfs[0])                             # src/Optimizer.cpp:266 ...
    kfs[0].Erase_MapPointMatch(mp)                           # ... :267 finds no index: the slot stays
    assert kfs[0].mvMapPoints[2] is mp and not mp.IsBad()
    return case("observation_erased_slot_still_set", b, [I12], n_local=1, quirk_point=mp.mlID)


def no_observation_left():                                   # d)
    b = Builder(4)
    kf0, kf1 = b.keyframe(6), b.keyframe(6)
    b.new_point(kf0, 0)
    lone = b.new_point(kf0, 1, observe=False)
    b.new_point(kf0, 2)
    b.link(kf1, 3, b.mps[0])
    return case("point_without_observation", b, [I12], n_local=2, lone_point=lone.mlID)


def bad_point():                                             # e)
    b = Builder(5).trajectory(6, 12, null=0.0)
    b.kfs[0].mvMapPoints[3].SetBadFlag()
    b.kfs[1].mvMapPoints[0].SetBadFlag()
    return case("bad_point_in_a_local_keyframe", b, [pose((-0.01, 0, 0))], n_local=3)


def found_changes():                                         # f)
    b = Builder(6).trajectory(8, 16)
    return case("found_counts_change", b, [pose((-0.05, 0, 0))], n_local=3, found_updates=[(0, 77), (5, 0), (len(b.mps) - 1, 2 ** 31 - 1), (9, -3)])


def growth():                                                # h)
    b = Builder(8, step=0.02).trajectory(70, 256, back=2)
    return case("grows_past_the_initial_capacities", b, [pose((-0.3, 0, 0)), pose((-1.2, 0, 0))], n_local=10, first_part=30)


def emitted(n_points, short_obs=False):                      # i)
    b = Builder(9)
    kf0, kf1 = b.keyframe(2048, x=0.0), b.keyframe(n_points - 2048, x=0.05)
    far = b.keyframe(600, x=0.5)
    for kf in (kf0, kf1):
        for s in range(len(kf.mvMapPoints)):
            b.new_point(kf, s)
    for s in range(600):
        b.link(far, s, b.mps[6 * s + 3])
    c = case(f"emits_{n_points}_points" + ("_one_observation_short" if short_obs else ""), b, [I12], n_local=2)
    if short_obs:
        c["obs_capacity"] = TR.track_map_local(CAM, I12, c["world"], 2)["n_obs"] - 1
    return c


def violated_duty():                                         # j)
    c = plain()
    w = c["world"]
    k = 3
    s_obs = int(np.flatnonzero(w["observes"][k])[-1])          # an observing slot near the end ...
    s_free = int(np.flatnonzero(w["slots"][k] < 0)[0])         # ... and a NULL slot in front of it
    assert s_free < s_obs
    w["slots"][k][s_free], w["observes"][k][s_free] = w["slots"][k][s_obs], 1
    c.update(name="two_observing_slots_of_one_keyframe", kfs=None, mps=None, twice=(k, s_free, s_obs), poses=[pose((-0.32, 0, 0))])
    return c


_CACHE = {}


def cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def small_cases():
    return cached("small", lambda: [plain(), outside_observers(), ba_quirk(), no_observation_left(), bad_point(), found_changes(), violated_duty()])


def all_cases():
    return cached("all", lambda: small_cases() + [growth(), emitted(4096), emitted(4097), emitted(4096, short_obs=True)])


def by_name(name):
    return [c for c in all_cases() if c["name"] == name][0]


def expected(c):
    """The restatement's answers, one per pose (computed once per session; never changed)."""
    return cached(("expected", c["name"]), lambda: [TR.track_map_local(CAM, T, c["world"], c["n_local"], 0, c["point_capacity"], c["obs_capacity"])
                                                    for T in c["poses"]])


def obs_capacity_of(c, want):
    return max(want["n_obs"], 1) if c["obs_capacity"] is None else c["obs_capacity"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    bits = BITS.get(a.dtype)
    return np.array_equal(a.view(bits), b.view(bits)) if bits else np.array_equal(a, b)


def same_columns(got, want, what):
    """Every column equal: integers equal, floats and doubles bit for bit (every value is a copy)."""
    for k in FLAT_KEYS:
        assert same_bits(got[k], want[k]), (what, k, got[k], want[k])


def same_answer(got, want, what):
    """The acceptance check of a whole answer: lists, counts and flags equal, kf_dist and every column bit-equal."""
    for k in ("n_close", "n_kf", "n_points", "n_obs", "overflow_points", "overflow_obs", "kf", "point", "point_kf"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert same_bits(np.array(got["kf_dist"], np.float64), np.array(want["kf_dist"], np.float64)), (what, got["kf_dist"], want["kf_dist"])
    same_columns(got["flat"], want["flat"], what)


def write_cases(path, cs):
    """The cases as tests/track_map_host/driver.cpp reads them."""
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(cs)))
        for c in cs:
            w = c["world"]
            P, K = len(w["p_world"]), len(w["slots"])
            ocap = c["file_obs_capacity"] if "file_obs_capacity" in c else max(obs_capacity_of(c, r) for r in expected(c))      # (its own: no restatement is run)
            f.write(struct.pack("6i", c["n_local"], c["point_capacity"], ocap, P, K, len(c["poses"])))
            f.write(np.ascontiguousarray(w["p_world"], np.float64).tobytes() + np.ascontiguousarray(w["bad"], np.uint8).tobytes())
            f.write(np.ascontiguousarray(w["found"], np.int32).tobytes() + np.ascontiguousarray(w["T_kf_w"], np.float64).tobytes())
            f.write(np.array([len(s) for s in w["slots"]], np.int32).tobytes())
            for key, dt in (("slots", np.int32), ("observes", np.uint8), ("px", np.float32), ("level", np.int32), ("bearing", np.float64)):
                for a in w[key]:
                    f.write(np.ascontiguousarray(a, dt).tobytes())
            f.write(np.array(c["poses"], np.float64).tobytes())


def read_answers(path, cs):
    """What the driver wrote: one answer per case and pose, in the form of the restatement's."""
    buf, at, out = open(path, "rb").read(), 0, []

    def take(dt, n):
        nonlocal at
        a = np.frombuffer(buf, dt, n, at).copy()
        at += a.nbytes
        return a
    for c in cs:
        per = []
        for _ in c["poses"]:
            n_close, n_kf, n_points, n_obs, m, no = (int(v) for v in take(np.int32, 6))
            ans = dict(n_close=n_close, n_kf=n_kf, n_points=n_points, n_obs=n_obs, overflow_points=int(n_points > m), overflow_obs=int(n_obs > no))
            ans["kf"], ans["kf_dist"] = take(np.int32, n_kf).tolist(), take(np.float64, n_kf).tolist()
            ans["point"], ans["point_kf"] = take(np.int32, m).tolist(), take(np.int32, m).tolist()
            ans["flat"] = dict(pw=take(np.float64, 3 * m).reshape(m, 3), found=take(np.int32, m), bad=take(np.uint8, m), off=take(np.int32, m + 1),
                               okf=take(np.int32, no), opx=take(np.float32, 2 * no).reshape(no, 2), olv=take(np.int32, no),
                               ob=take(np.float64, 3 * no).reshape(no, 3))
            per.append(ans)
        out.append(per)
    assert at == len(buf)
    return out
