"""The cases of dsdtm_localmap_select (include/dsdtm_amd_localmap.h, rules L1-L4), shared by the CPU and the GPU half of the tests: the
smallest maps at which the selection can go wrong. A case is a dict: name, world (the restatement's map: p_world, bad, T_kf_w,
slots), poses (12 doubles each), n_local, boundary, capacity (None: room for the whole list). expected(case) is the restatement's
answer per pose, computed once per session. Test infrastructure only."""
import math
import struct
from types import SimpleNamespace

import numpy as np

from dsdtm_amd import local_map_restatement as R

CAM = SimpleNamespace(fx=np.float32(512.0), fy=np.float32(512.0), cx=np.float32(320.0), cy=np.float32(240.0), f=np.float32(512.0), width=640, height=480)
I12 = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


def pose(t=(0.0, 0.0, 0.0), yaw=0.0):
    c, s = math.cos(yaw), math.sin(yaw)
    return [c, 0.0, -s, float(t[0]), 0.0, 1.0, 0.0, float(t[1]), s, 0.0, c, float(t[2])]


def at_pixel(u=320.0, v=240.0, z=2.0):
    """A world point that the identity pose projects to (u, v) (up to rounding) at depth z."""
    return ((u - 320.0) / 512.0 * z, (v - 240.0) / 512.0 * z, z)


BEHIND = (0.0, 0.0, -5.0)        # z < 0 for the identity pose: never visible


class Builder:
    def __init__(self):
        self.p, self.bad, self.T, self.slots = [], [], [], []

    def point(self, X, bad=0):
        self.p.append([float(v) for v in X])
        self.bad.append(int(bad))
        return len(self.p) - 1

    def kf(self, slots, t=(0.0, 0.0, 0.0)):
        self.T.append(pose(t))
        self.slots.append(np.array(list(slots), np.int32))
        return len(self.T) - 1

    def world(self):
        return dict(p_world=np.array(self.p, np.float64).reshape(-1, 3), bad=np.array(self.bad, np.uint8),
                    T_kf_w=np.array(self.T, np.float64).reshape(-1, 12), slots=[s.copy() for s in self.slots])


def case(name, b, poses=(I12,), n_local=10, boundary=0, capacity=None):
    return dict(name=name, world=b.world() if isinstance(b, Builder) else b, poses=[list(p) for p in poses], n_local=n_local, boundary=boundary,
                capacity=capacity)


def degenerate_cases():
    out = [case("empty_map", Builder())]
    b = Builder()
    b.kf([b.point(at_pixel())])
    out.append(case("one_keyframe_one_slot", b))
    b = Builder()
    b.kf([])
    b.kf([b.point(at_pixel(100, 100))], t=(1, 0, 0))
    b.kf([])
    out.append(case("keyframes_without_slots", b))
    b = Builder()
    b.point(at_pixel())
    out.append(case("points_but_no_keyframe", b))
    return out


def chunk_tail_cases():
    out = []
    for ns in (63, 64, 65, 129):
        b = Builder()
        hidden = [b.point(BEHIND) for _ in range(3)]
        seen = b.point(at_pixel(7, 9))
        slots = [(-1 if i % 3 == 0 else hidden[i % 3]) for i in range(ns - 1)] + [seen]
        b.kf(slots, t=(0.5, 0, 0))
        b.kf([(-1 if i % 2 else hidden[0]) for i in range(ns)], t=(0.25, 0, 0))      # nothing visible at the same length
        out.append(case(f"only_visible_point_in_last_of_{ns}_slots", b))
    return out


def rule_one_cases():
    out = []
    for zero in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)):
        b = Builder()
        b.kf([b.point(zero)])                               # with t = (0, 0, 2) it projects to the principal point
        b.kf([b.point((0.0, 0.0, 1e-300))], t=(1, 0, 0))     # not exactly zero: visible
        out.append(case("zero_position_%s" % ("neg" if math.copysign(1.0, zero[0]) < 0 else "pos"), b, poses=[pose((0, 0, 2))]))
    b = Builder()
    p = b.point(at_pixel(50, 60), bad=1)
    b.kf([p, b.point(BEHIND)])
    out.append(case("only_visible_point_is_bad", b))
    b = Builder()
    b.kf([b.point((0.1, 0.0, -1e-9))])                       # z < 0
    b.kf([b.point((0.1, 0.0, 0.0))])                         # z == 0: u infinite
    b.kf([b.point((0.0, 0.0, 0.0 + 5e-324)), b.point((1.0, 0.0, 1e-12))])      # z tiny: u = 320 (x = 0) visible; |u| >= 1e9 not
    b.kf([b.point((1.0, 0.0, 1e-12))])
    b.kf([b.point((1.0, 1.0, 512.0 / (1e9 - 320.0)))])       # u just about 1e9
    out.append(case("depth_guards", b, n_local=64))
    return out


def edge_cases():
    out = []
    w, h = CAM.width, CAM.height
    for boundary in (0, 8):
        for axis, size in (("u", w), ("v", h)):
            vals = [-0.5, 0.5, size - 1.5, size - 0.5, boundary - 0.5, boundary + 0.5, size - boundary - 1.5, size - boundary - 0.5]
            for k in (10, 11, boundary, size - boundary - 1):
                vals += [k + 0.5 - 1e-9, k + 0.5 + 1e-9, k - 0.5 + 1e-9, k - 0.5 - 1e-9, k + 0.5 - 1e-4, k + 0.5 + 1e-4]
            b = Builder()
            for i, val in enumerate(vals):
                X = at_pixel(val, 200.0, 1.0) if axis == "u" else at_pixel(300.0, val, 1.0)
                b.kf([b.point(X)], t=(0.001 * i, 0, 0))
            out.append(case(f"edges_{axis}_boundary_{boundary}", b, n_local=64, boundary=boundary))
    return out


def selection_cases():
    out = []

    def ring(dists, visible=None):
        b = Builder()
        for i, d in enumerate(dists):
            vis = visible is None or visible[i]
            b.kf([b.point(at_pixel(20 + i, 30) if vis else BEHIND), b.point(at_pixel(21 + i, 31))] if vis else [b.point(BEHIND)], t=(d, 0, 0))
        return b
    out.append(case("two_identical_translations", ring([2.0, 1.0, 1.0, 3.0]), n_local=3))
    out.append(case("tie_at_the_cut", ring([3.0, 1.0, 3.0, 2.0, 3.0, 0.5]), n_local=4))
    out.append(case("tie_at_the_cut_negative_side", ring([-3.0, 1.0, 3.0, 2.0, -3.0, 0.5]), n_local=4))
    out.append(case("exactly_n_local_close", ring([5, 4, 3, 2, 1], [1, 0, 1, 1, 0]), n_local=3))
    out.append(case("fewer_close_than_n_local", ring([5, 4, 3, 2, 1], [0, 0, 1, 1, 0]), n_local=3))
    out.append(case("more_close_than_n_local", ring([5, 4, 3, 2, 1, 0.5, 7]), n_local=3))
    out.append(case("n_local_1", ring([5, 4, 0.25, 2, 0.25]), n_local=1))
    out.append(case("n_local_64_of_70", ring([((i * 37) % 70) * 0.125 for i in range(70)]), n_local=64))
    out.append(case("n_local_64_of_300_with_ties", ring([((i * 7) % 25) * 0.5 for i in range(300)], [i % 3 != 1 for i in range(300)]), n_local=64))
    return out


def duplicate_cases():
    out = []
    b = Builder()
    shared, own0, own1, lone = b.point(at_pixel(10, 10)), b.point(at_pixel(11, 10)), b.point(at_pixel(12, 10)), b.point(at_pixel(13, 10))
    b.kf([own1, shared, -1], t=(2, 0, 0))        # chosen second: `shared` is listed by the nearer keyframe first
    b.kf([shared, own0], t=(1, 0, 0))
    b.kf([lone, shared], t=(3, 0, 0))            # not chosen with n_local = 2: `lone` is absent
    out.append(case("point_in_two_chosen_keyframes", b, n_local=2))
    b = Builder()
    pts = [b.point(at_pixel(5 + i % 600, 5 + i // 600)) for i in range(400)]
    slots = list(pts[:340])
    slots[3] = pts[1]            # twice within one 64-entry chunk
    slots[60] = pts[59]          # neighbours
    slots[70] = pts[2]           # across wavefronts of one 256-entry chunk
    slots[300] = pts[0]          # 300 slots apart: another 256-entry chunk
    slots[339] = pts[338]
    slots[255], slots[256] = pts[254], pts[254]      # across the chunk border
    b.kf(slots, t=(1, 0, 0))
    b.kf([pts[399], pts[0], pts[399], pts[398], pts[340]] * 3, t=(2, 0, 0))
    out.append(case("duplicates_within_a_keyframe", b, n_local=2))
    return out


def capacity_cases():
    out = []
    for name, short in (("capacity_one_short", 1), ("capacity_zero", None)):
        b = Builder()
        pts = [b.point(at_pixel(30 + i, 40), bad=(i % 11 == 5)) for i in range(300)]
        b.kf(pts[:200], t=(1, 0, 0))
        b.kf(pts[150:], t=(2, 0, 0))
        c = case(name, b, n_local=2)
        full = R.select_local_map(CAM, I12, c["world"], 2, 0)["n_points"]
        c["capacity"] = full - 1 if short else 0
        out.append(c)
    return out


def random_world(seed=5, n_kf=300, n_slots=200, n_points=20000, n_poses=8):
    """Keyframes on a ring around the origin, each listing points of its own neighbourhood (some shared with its neighbours, some
    NULL slots, some bad points, some listed twice); poses at the origin looking around: a minority of the keyframes is close."""
    rng = np.random.default_rng(seed)
    per = n_points // n_kf
    ang = np.arange(n_kf) * (2 * math.pi / n_kf)
    centre = np.stack([8.0 * np.sin(ang), np.zeros(n_kf), 8.0 * np.cos(ang)], 1)
    p = np.repeat(centre, per, 0) + rng.uniform(-0.4, 0.4, (n_kf * per, 3))
    p = np.vstack([p, rng.uniform(-10, 10, (n_points - len(p), 3))])
    bad = (rng.random(n_points) < 0.05).astype(np.uint8)
    T, slots = [], []
    for k in range(n_kf):
        own = np.arange(k * per, (k + 1) * per)
        nb = np.arange(((k + 1) % n_kf) * per, ((k + 1) % n_kf) * per + per // 2)
        s = rng.choice(np.concatenate([own, nb, nb[:10], own[:20]]), n_slots).astype(np.int32)
        s[rng.random(n_slots) < 0.2] = -1
        slots.append(s)
        T.append(pose(tuple(rng.integers(-8, 9, 3) * 0.25)))        # a coarse lattice: equal distances occur
    poses = [pose(tuple(rng.integers(-4, 5, 3) * 0.25), yaw=i * 2 * math.pi / n_poses + 0.1) for i in range(n_poses)]
    return case("random_world", dict(p_world=p, bad=bad, T_kf_w=np.array(T), slots=slots), poses=poses, n_local=10)


def small_cases():
    return degenerate_cases() + chunk_tail_cases() + rule_one_cases() + edge_cases() + selection_cases() + duplicate_cases() + capacity_cases()


_CACHE = {}


def cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def all_cases():
    return cached("all", lambda: small_cases() + [random_world()])


def expected(c):
    """The restatement's answers, one per pose (computed once per session; never changed)."""
    return cached(("expected", c["name"]), lambda: [R.select_local_map(CAM, T, c["world"], c["n_local"], c["boundary"], c["capacity"]) for T in c["poses"]])


def write_cases(path, cs):
    """The cases as tests/local_map_host/driver.cpp reads them. A case may bring its own `file_capacity` (no restatement is run then)."""
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(cs)))
        for c in cs:
            w = c["world"]
            P, K = len(w["p_world"]), len(w["slots"])
            cap = c["file_capacity"] if "file_capacity" in c else c["capacity"] if c["capacity"] is not None else max(1, max(r["n_points"] for r in expected(c)))
            f.write(struct.pack("6i", c["n_local"], c["boundary"], cap, P, K, len(c["poses"])))
            f.write(np.ascontiguousarray(w["p_world"], np.float64).tobytes())
            f.write(np.ascontiguousarray(w["bad"], np.uint8).tobytes())
            f.write(np.ascontiguousarray(w["T_kf_w"], np.float64).tobytes())
            f.write(np.array([len(s) for s in w["slots"]], np.int32).tobytes())
            for s in w["slots"]:
                f.write(np.ascontiguousarray(s, np.int32).tobytes())
            f.write(np.array(c["poses"], np.float64).tobytes())


def capacity_of(c, want):
    return max(want["n_points"], 1) if c["capacity"] is None else c["capacity"]


def same_answer(got, want, what):
    """The acceptance check: lists and counters equal, distances bit-equal (no tolerance: every operation is correctly rounded)."""
    for k in ("n_close", "n_kf", "n_points", "overflow", "kf", "point", "point_kf"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(np.array(got["kf_dist"], np.float64).view(np.uint64), np.array(want["kf_dist"], np.float64).view(np.uint64)), (what, got["kf_dist"], want["kf_dist"])
