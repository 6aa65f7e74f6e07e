"""The worlds of libdsdtm_amd_mapping.so (include/dsdtm_amd_mapping.h), shared by the CPU and the GPU half of its tests: small maps built
from the objects of tests/track_map_cases.py (at most 24 keyframes of at most 48 slots, except the limit cases), one case per rule edge.
A case is a dict: name, worlds (track_map_restatement's; `objects` holds the (kfs, mps) they came from), and what is asked of them:
    cov       [(world, kf, capacity or None)]                           dsdtm_mapping_covisibility
    windows   [(world, kf, cov_kf, origin_kf, kcap, pcap, ocap)]        dsdtm_mapping_ba_window (a capacity of None: room for all)
    outliers  {window: [(map point, map keyframe)]} or None             dsdtm_mapping_ba_commit with hand-set flags (None: no commit)
    overlap   (first, second) when the commit must be refused
expected(case) is the restatement's answer, computed once per session and never changed. Test infrastructure only."""
import numpy as np

from dsdtm_amd import ba_window_restatement as BR
from tests.track_map_cases import Builder, cached, same_bits, world_of

ROOM = dict(kcap=80, pcap=512, ocap=2048)      # "room for all" on the device, for the small worlds


class World(Builder):
    """track_map_cases.Builder with a next free slot per keyframe."""

    def __init__(self, seed):
        super().__init__(seed)
        self.free = []

    def kf(self, n_slots=48):
        self.free.append(0)
        return self.keyframe(n_slots)

    def slot(self, kf):
        self.free[kf.mlId] += 1
        return self.free[kf.mlId] - 1

    def point(self, kf, observe=True):
        return self.new_point(kf, self.slot(kf), observe)

    def see(self, kf, mp, observe=True):
        self.link(kf, self.slot(kf), mp, observe)

    def share(self, a, b, n):
        """n new points observed by keyframes a and b."""
        return [self.see(b, mp) or mp for mp in [self.point(a) for _ in range(n)]]

    def world(self):
        return world_of(self.kfs, self.mps)


def case(name, builders, cov=(), windows=(), outliers=None, overlap=None):
    return dict(name=name, worlds=[b.world() for b in builders], objects=[(b.kfs, b.mps) for b in builders], cov=list(cov), windows=list(windows),
                outliers=outliers, overlap=overlap)


# ---- covisibility -----------------------------------------------------------------------------------------------------------------

def cov_threshold():
    b = World(11)
    k = [b.kf() for _ in range(3)]
    b.share(k[0], k[1], 15)
    b.share(k[0], k[2], 16)
    return case("cov_weight_15_is_out_16_is_in", [b], cov=[(0, 0, 8)])


def cov_fallback_tie():
    b = World(12)
    k = [b.kf() for _ in range(4)]
    b.share(k[0], k[3], 3)
    b.share(k[0], k[2], 5)
    b.share(k[0], k[1], 5)
    return case("cov_none_above_15_tie_lowest_index", [b], cov=[(0, 0, 8), (0, 3, 8)])


def cov_nothing_shared():
    b = World(13)
    for kf in [b.kf(8) for _ in range(3)]:
        for _ in range(5):
            b.point(kf)
    return case("cov_no_shared_point", [b], cov=[(0, 1, 4)])


def cov_listed_twice_unobserved_and_bad():
    b = World(14)
    k = [b.kf() for _ in range(4)]
    twice = b.share(k[0], k[1], 3)[0]
    b.see(k[0], twice, observe=False)                       # a second slot of kf 0 lists the point: it counts twice
    lone = b.point(k[2])
    b.see(k[0], lone, observe=False)                        # listed by kf 0, not observed by it: still counts for kf 2
    bad = b.share(k[0], k[3], 4)[1]
    bad.SetBadFlag()                                        # (the flag alone: its observations stay, and it must not count)
    return case("cov_listed_twice_listed_unobserved_bad_point", [b], cov=[(0, 0, 8)])


def cov_equal_weights():
    b = World(15)
    k = [b.kf() for _ in range(5)]
    b.share(k[0], k[3], 16)
    b.share(k[0], k[1], 16)
    b.share(k[0], k[2], 16)
    return case("cov_equal_weights_sort_by_index_and_overflow", [b], cov=[(0, 0, 8), (0, 0, 2), (0, 0, 0)])


# ---- window ------------------------------------------------------------------------------------------------------------------------

def window_world(seed=21):
    """Six keyframes; tKFrame is 5 with the covisible 3 and 4. The fixed keyframes appear in the order 2, 1, 0."""
    b = World(seed)
    k = [b.kf() for _ in range(6)]
    b.share(k[5], k[2], 1)                                  # the first local point has an outside observer: keyframe 2 is the first fixed one
    b.share(k[5], k[4], 6)                                  # listed by two local keyframes: emitted once, at keyframe 5's place
    b.share(k[5], k[3], 4)
    b.share(k[5], k[1], 1)
    b.share(k[4], k[3], 3)
    b.share(k[4], k[0], 2)
    b.see(k[4], b.point(k[0]), observe=False)               # listed by a local keyframe that does not observe it: still a local point
    for kf in k:
        b.point(kf)
    b.share(k[1], k[0], 3)                                  # nothing local sees these
    return b


def window_basic():
    return case("window_first_occurrence_fixed_order_listed_unobserved", [window_world()], windows=[(0, 5, [3, 4], -1, None, None, None)], outliers={0: []})


def window_origin():
    b = window_world()
    return case("window_kf_is_origin_no_points_and_origin_in_cov_is_constant", [b],
                windows=[(0, 5, [3, 4], 5, None, None, None), (0, 5, [3, 4], 3, None, None, None), (0, 5, [], -1, None, None, None), (0, 5, [], 5, None, None, None)])


def window_short_capacities():
    b = window_world()
    full = BR.ba_window(b.world(), 5, [3, 4])
    nk, npt, no = full["n_local"] + full["n_fixed"], full["n_points"], full["n_obs"]
    return case("window_each_capacity_short_by_one", [b], windows=[(0, 5, [3, 4], -1, nk - 1, npt, no), (0, 5, [3, 4], -1, nk, npt - 1, no),
                                                                      (0, 5, [3, 4], -1, nk, npt, no - 1), (0, 5, [3, 4], -1, nk, npt, no)])


def window_two_on_one_map_two_maps():
    a, b = window_world(), window_world(22)
    b.share(b.kfs[2], b.kfs[0], 4)
    return case("window_two_windows_on_one_map_and_two_maps", [a, b], windows=[(0, 5, [3, 4], -1, None, None, None), (0, 2, [1], 0, None, None, None),
                                                                                 (1, 4, [5, 2], -1, None, None, None)])


def window_free_limit():
    b = World(23)
    k = [b.kf(4) for _ in range(17)] + [b.kf(24)]
    for kf in k:
        b.point(kf)
    for kf in k[:17]:
        b.see(kf, b.point(k[17]))
    return case("window_16_and_17_free_keyframes", [b], windows=[(0, 17, list(range(15)), -1, None, None, None), (0, 17, list(range(16)), -1, None, None, None),
                                                                  (0, 17, list(range(16)), 0, None, None, None)])


def window_fixed_limit(n_fixed):
    b = World(24)
    first = b.kf(n_fixed)                                   # (a limit case: more than 24 keyframes, more than 48 slots)
    for _ in range(n_fixed):
        b.see(b.kf(1), b.point(first))
    return case(f"window_{n_fixed}_fixed_keyframes", [b], windows=[(0, 0, [], -1, None, None, None)])


# ---- commit ------------------------------------------------------------------------------------------------------------------------

def commit_world():
    """tKFrame 3 with the covisible 2; 0 and 1 are fixed. Points by observers: A 1,2,3; B 2,3; C 0,2,3; D 1,2,3; E 3; F 1,2,3."""
    b = World(31)
    k = [b.kf(12) for _ in range(4)]
    pts = {}
    for name, others in (("A", (2, 1)), ("B", (2,)), ("C", (2, 0)), ("D", (2, 1)), ("E", ()), ("F", (2, 1))):
        mp = b.point(k[3])
        for o in others:
            b.see(k[o], mp)
        pts[name] = mp.mlID
    b.share(k[1], k[0], 2)
    return b, pts


def commit_case(name, flags):
    b, p = commit_world()
    return case("commit_" + name, [b], windows=[(0, 3, [2], -1, None, None, None)], outliers={0: [(p[n], k) for n, k in flags]})


def commit_cases():
    return [commit_case("no_outlier", []),
            commit_case("one_of_three_point_stays_good", [("A", 2)]),
            commit_case("one_of_two_point_goes_bad", [("B", 2)]),
            commit_case("two_of_three_bad_after_the_second", [("C", 0), ("C", 3)]),
            commit_case("three_of_three_third_changes_nothing", [("D", 1), ("D", 2), ("D", 3)]),
            commit_case("single_observation_is_an_outlier", [("E", 3)]),
            commit_case("all_of_them_together", [("A", 2), ("B", 2), ("C", 0), ("C", 3), ("D", 1), ("D", 2), ("D", 3), ("E", 3)])]


def commit_overlap():
    b, p = commit_world()
    return case("commit_two_overlapping_windows_refused", [b], windows=[(0, 1, [0], -1, None, None, None), (0, 3, [2], -1, None, None, None), (0, 2, [3], -1, None, None, None)],
                outliers={0: [], 1: [(p["B"], 2)], 2: []}, overlap=(0, 1))


# ---- the chain through the solver --------------------------------------------------------------------------------------------------------

def chain_world():
    """A window of tests/local_ba_restatement.make_world as a map: keyframe k's slots are its observations in point order (each
    observes), tKFrame is keyframe 0 with the other free keyframes as its covisible ones, the rest are fixed. Chosen (and asserted by
    tests/test_ba_window_cpu.py on the CPU and by the GPU chain test) so that the solve flags outliers, at least one point goes bad
    and at least one point with an outlier stays good. Returns (world, kf, cov_kf, delta)."""
    def make():
        from tests import local_ba_restatement as R
        n_free = 3
        w = R.make_world(41, n_free=n_free, n_fixed=3, n_points=60, outlier_frac=0.12, once_frac=0.0, max_obs=5)
        K = len(w.T)
        slots = [[] for _ in range(K)]
        feats = [[] for _ in range(K)]
        for j in np.argsort(w.obs_pt, kind="stable"):
            slots[w.obs_kf[j]].append(int(w.obs_pt[j]))
            feats[w.obs_kf[j]].append((w.bearing[j], int(w.level[j])))
        world = dict(p_world=w.points.copy(), bad=np.zeros(len(w.points), np.uint8), found=np.ones(len(w.points), np.int32),
                     T_kf_w=w.T.reshape(K, 12).copy(), slots=[np.array(s, np.int32) for s in slots],
                     observes=[np.ones(len(s), np.uint8) for s in slots], px=[np.zeros((len(s), 2), np.float32) for s in slots],
                     level=[np.array([l for _, l in f], np.int32) for f in feats],
                     bearing=[np.array([b for b, _ in f], np.float64).reshape(-1, 3) for f in feats])
        return world, 0, list(range(1, n_free)), w.delta
    return cached("ba_window_chain_world", make)


def chain_property(win, outlier, commit):
    """What the chain world is chosen for: (outliers, points that went bad, points with an outlier that stayed good)."""
    hit = set(win["point_index"][win["obs_point"][np.flatnonzero(outlier)]].tolist())
    return int(np.count_nonzero(outlier)), commit["n_bad"], len(hit - set(commit["bad_points"]))


def all_cases():
    return cached("ba_window_all", lambda: [cov_threshold(), cov_fallback_tie(), cov_nothing_shared(), cov_listed_twice_unobserved_and_bad(), cov_equal_weights(),
                                            window_basic(), window_origin(), window_short_capacities(), window_two_on_one_map_two_maps(), window_free_limit(),
                                            window_fixed_limit(64), window_fixed_limit(65)] + commit_cases() + [commit_overlap()])


def by_name(name):
    return [c for c in all_cases() if c["name"] == name][0]


def flags_of(window, pairs):
    """Hand-set outlier flags of a usable window: observation j is an outlier when (its map point, its map keyframe) is in `pairs`."""
    want = set(pairs)
    return np.array([int((int(window["point_index"][window["obs_point"][j]]), int(window["obs_slot"][j]) >> 32) in want) for j in range(len(window["obs_point"]))], np.uint8)


def expected(c):
    """The restatement's answers: cov (one per pair), windows (one per window), and, with outliers, flags / commits per window (None for
    a window that is not usable), overlap, and the worlds after the commit."""
    def make():
        e = dict(cov=[BR.update_connection(c["worlds"][w], kf, cap) for w, kf, cap in c["cov"]],
                 windows=[BR.ba_window(c["worlds"][w], kf, cov, origin, kc, pc, oc) for w, kf, cov, origin, kc, pc, oc in c["windows"]])
        if c["outliers"] is not None:
            e["flags"] = [flags_of(win, c["outliers"].get(i, [])) if win["usable"] else None for i, win in enumerate(e["windows"])]
            e["overlap"] = BR.overlap([(c["windows"][i][0], win) for i, win in enumerate(e["windows"])])
            worlds, e["commits"] = list(c["worlds"]), []
            for i, win in enumerate(e["windows"]):
                if e["overlap"] or not win["usable"]:
                    e["commits"].append(None)
                    continue
                m = c["windows"][i][0]
                worlds[m], r = BR.ba_commit(worlds[m], win, win["T_c2w"], win["points"], e["flags"][i])
                e["commits"].append(r)
            e["worlds_after"] = worlds
        return e
    return cached(("ba_window_expected", c["name"]), make)


WINDOW_COLUMNS = ("kf_index", "kf_constant", "T_c2w", "point_index", "points", "obs_kf", "obs_point", "obs_slot", "obs_bearing", "obs_level")


def same_window(got, want, what):
    for f in ("n_local", "n_fixed", "n_points", "n_obs", "usable") + BR.FLAGS:
        assert got[f] == want[f], (what, f, got[f], want[f])
    if want["usable"]:
        for k in WINDOW_COLUMNS:
            assert same_bits(np.asarray(got[k]).reshape(np.asarray(want[k]).shape), want[k]), (what, k, got[k], want[k])


def same_world(got, want, what):
    """Two worlds equal byte for byte (a map read back against the restated one)."""
    for k in ("p_world", "bad", "found", "T_kf_w"):
        assert same_bits(np.asarray(got[k]), np.asarray(want[k]).astype(np.asarray(got[k]).dtype)), (what, k)
    for k in ("slots", "observes", "px", "level", "bearing"):
        assert len(got[k]) == len(want[k]), (what, k)
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert same_bits(np.asarray(a), np.asarray(b).astype(np.asarray(a).dtype).reshape(np.asarray(a).shape)), (what, k, i, a, b)
