"""The worlds of libdsdtm_amd_mapping.so (include/dsdtm_amd_mapping.h), shared by the CPU and the GPU half of its tests. Two lists:
all_cases() — small maps built from the objects of tests/track_map_cases.py (at most 24 keyframes of at most 48 slots, except the
limit cases), one case per rule edge — and size_cases() — maps sized past the kernels' loop boundaries: keyframes of up to 4096 slots,
up to 257 keyframes, windows of up to 700 entries, 76 keyframes and about 1000 observations, and point indices chosen by the kernels'
hashes so that the two open-addressing tables chain, wrap and miss; one case per boundary, named for it. Every world is generated from
a seed in the process. A size world is built from objects where sequential point indices do, and as plain arrays (Arrays, `objects`
holds (None, None)) where the indices are chosen.
A case is a dict: name, worlds (track_map_restatement's; `objects` holds the (kfs, mps) they came from), and what is asked of them:
    cov       [(world, kf, capacity or None)]                           dsdtm_mapping_covisibility
    windows   [(world, kf, cov_kf, origin_kf, kcap, pcap, ocap)]        dsdtm_mapping_ba_window (a capacity of None: room for all)
    outliers  {window: [(map point, map keyframe)]} or None             dsdtm_mapping_ba_commit with hand-set flags (None: no commit)
    overlap   (first, second) when the commit must be refused
    room      the device capacities that stand for "room for all"; bad_capacity of the commit (None: room for all)
expected(case) is the restatement's answer, computed once per session and never changed. Test infrastructure only."""
from collections import Counter

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


def case(name, builders, cov=(), windows=(), outliers=None, overlap=None, room=ROOM, bad_capacity=None):
    return dict(name=name, worlds=[b.world() for b in builders], objects=[(b.kfs, b.mps) for b in builders], cov=list(cov), windows=list(windows),
                outliers=outliers, overlap=overlap, room=room, bad_capacity=bad_capacity)


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


# ---- size worlds: past one wavefront (64), one workgroup (256), 64 keyframes per workgroup, and the ends of the two hash tables ---------

BIG_ROOM = dict(kcap=80, pcap=1024, ocap=4096)
MULTIPLIER = 2654435761


# The two hashes of csrc/mapping.hip, restated: cov_home is mp_hash13 (the covisibility table in LDS, 8192 cells), win_home is mp_hash
# (the first-occurrence table of a window, 2^bits cells). The worlds below choose point indices by them, and the CPU property checks
# model the tables with them: if a kernel's hash ever stops matching its restatement here, those checks cannot notice — the worlds
# would still be answered correctly, but no longer chain, wrap or miss where their names say.
def cov_home(p):
    return ((p * MULTIPLIER) % 2 ** 32) >> 19


def win_home(p, bits):
    return ((p * MULTIPLIER) % 2 ** 32) >> (32 - bits)


def table_bits(E):
    """T_bits of a window with E entries: the smallest number of bits, from 4 up, with 2^bits >= 2E."""
    bits = 4
    while (1 << bits) < 2 * E:
        bits += 1
    return bits


def probe_table(points, home, size):
    """The model of either table: {cell: point} after the distinct points were inserted by linear probing. WHICH cells are taken does
    not depend on the order of insertion (so it is what the device's table holds too); which point sits in which cell of a chain does."""
    cells = {}
    for p in points:
        if p in cells.values():
            continue
        h = home(p)
        while h in cells:
            h = (h + 1) % size
        cells[h] = p
    return cells


def probe_find(cells, home, size, p):
    """(the cell of p or -1, the cells looked at): a probe ends at p or at an empty cell."""
    h, walk = home(p), []
    while h in cells:
        walk.append(h)
        if cells[h] == p:
            return h, walk
        h = (h + 1) % size
    return -1, walk + [h]


def cov_listed(world, kf):
    """The points of keyframe kf's slots that the covisibility table holds (set, not bad), in slot order, repeated as listed."""
    return [int(p) for p in world["slots"][kf] if p >= 0 and not world["bad"][p]]


def cov_weights(world, kf):
    """{keyframe: weight} of UpdateConnection, counted slot by slot (no set, no table): the property checks' own count."""
    mult, out = Counter(cov_listed(world, kf)), {}
    for k, (slots, obs) in enumerate(zip(world["slots"], world["observes"])):
        w = sum(int(mult.get(int(p), 0)) for p, o in zip(slots, obs) if o and p >= 0)
        if k != kf and w:
            out[k] = w
    return out


def entries(world, kf, cov):
    """The entries of a window in order: the slots of tKFrame, then of each covisible keyframe (a point index or -1)."""
    return [int(p) for k in [kf] + list(cov) for p in world["slots"][k]]


class Arrays:
    """A world as plain arrays, for the cases whose point indices are chosen: keyframes are lists of point indices (-1: a NULL slot)."""
    kfs = mps = None

    def __init__(self, seed, n_points):
        self.seed, self.rng, self.P, self.slots, self.observes, self.bad = seed, np.random.default_rng(seed), n_points, [], [], np.zeros(n_points, np.uint8)

    def kf(self, slots, observes=None):
        """A keyframe; every set slot observes unless `observes` says otherwise. Returns its index."""
        s = np.array(slots, np.int32).reshape(-1)
        self.slots.append(s)
        self.observes.append((s >= 0).astype(np.uint8) if observes is None else np.array(observes, np.uint8).reshape(-1) & (s >= 0))
        return len(self.slots) - 1

    def world(self):
        K = len(self.slots)
        T = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64), (K, 1))
        T[:, 3] = -0.125 * np.arange(K)
        draw = lambda k, column: np.random.default_rng([self.seed, k, column])       # (a slot's features depend on (keyframe, slot) alone: siblings agree)
        bearing = []
        for k, s in enumerate(self.slots):
            n = draw(k, 0).normal(size=(len(s), 3))
            bearing.append(n / np.linalg.norm(n, axis=1, keepdims=True))
        return dict(p_world=draw(len(self.slots), 3).uniform(-2.0, 2.0, (self.P, 3)), bad=self.bad.copy(), found=np.ones(self.P, np.int32), T_kf_w=T,
                    slots=[s.copy() for s in self.slots], observes=[o.copy() for o in self.observes],
                    px=[draw(k, 1).uniform(1, 400, (len(s), 2)).astype(np.float32) for k, s in enumerate(self.slots)],
                    level=[draw(k, 2).integers(0, 4, len(s)).astype(np.int32) for k, s in enumerate(self.slots)], bearing=bearing)


def cov_wide_keyframes():
    """kf 0 has 300 slots (two trips of the 256-thread fill loop) and lists one point in both trips; keyframes 1, 2, 3 have 64, 65 and
    130 slots, each with its LAST slot observing a point of kf 0 (slots 255, 256 and 299 of it). Weights: 15, 16 and 20."""
    b = World(61)
    k = [b.kf(n) for n in (300, 64, 65, 130, 40)]
    mine = [b.new_point(k[0], s) for s in range(270)]                                # by slot of keyframe 0
    b.link(k[0], 270, mine[10], observe=False)                                       # slots 10 and 270: it counts twice
    mine += [mine[10]] + [b.new_point(k[0], s) for s in range(271, 300)]

    def observe(kf, pairs):
        for s, s0 in pairs:
            b.link(kf, s, mine[s0])
    observe(k[1], [(s, 20 + s) for s in range(14)] + [(63, 255)])
    observe(k[2], [(s, 40 + s) for s in range(15)] + [(64, 256)])
    observe(k[3], [(60 + s, 100 + s) for s in range(11)] + [(5, 10), (129, 299)] + [(120 + s, 280 + s) for s in range(6)])
    for kf in k[1:]:
        for s in range(20, 30):
            b.new_point(kf, s)
    return case("cov_wide_keyframes", [b], cov=[(0, 0, 8), (0, 3, 8)])


def cov_K_world(K):
    """K keyframes around two hubs, keyframe 0 and keyframe K - 1. Against hub 0, keyframes 5, K - 57, K - 1 and K // 2 + 1 weigh 16, 17,
    17 and 18, every other one 1..3; against hub K - 1, keyframes 3, 0 and K - 2 weigh 16, 17 and 20. With K = 257 keyframe 1 is a
    third hub with nothing above 15: keyframes 130 and 256 both weigh 11, keyframe 2 weighs 3."""
    b = World(60 + K)
    k = [b.kf(3 * K + 100)] + [b.kf(48) for _ in range(K - 2)] + [b.kf(3 * K + 100)]
    over = {5: 16, K - 57: 17, K - 1: 17, K // 2 + 1: 18}
    for i in range(1, K):
        b.share(k[0], k[i], over.get(i, 1 + i % 3))
    over = {3: 16, K - 2: 20}
    for i in range(1, K - 1):
        b.share(k[K - 1], k[i], over.get(i, 1 + i % 2))
    if K == 257:
        b.share(k[1], k[256], 9)                                                     # + the 2 it shares with that hub already
        b.share(k[1], k[130], 11)
        b.share(k[1], k[2], 3)
    return b


def cov_K(K):
    pairs = [(0, 0, 8), (0, 0, 3), (0, K - 1, 8), (0, K - 1, 2)]
    if K == 257:                                                                     # the fallback: room for the one it names, and none
        pairs += [(0, 1, 8), (0, 1, 0)]
    worlds = [cov_K_world(K)]
    if K == 65:                                                                      # a 64-keyframe map in the same call: its second workgroup has no keyframe
        worlds.append(cov_K_world(64))
        pairs += [(1, 0, 8), (1, 63, 8)]
    return case(f"cov_K_{K}", worlds, cov=pairs)


def cov_table_chains():
    """24 000 points, indices chosen by cov_home. kf 0 lists four good points of one home cell H (a chain H .. H + 3), a bad point whose
    home is H + 1 (inside the chain: not inserted), both points whose home is cell 8191 and one whose home is cell 0 (a chain 8191, 0,
    1), and twelve points elsewhere. Keyframe 1 observes the chain at H, the bad point, a fifth point of home H that is NOT listed
    (its probe walks the chain to the empty cell H + 4), one point of the wrapping chain and the twelve: 4 + 1 + 12 = 17. Keyframe 2
    observes the wrapping chain and an unlisted point of home 0 (its probe ends at the empty cell 2): 3."""
    P = 24000
    homes = {}
    for p in range(P):
        homes.setdefault(cov_home(p), []).append(p)
    H = [h for h in sorted(homes) if 100 < h < 8000 and len(homes[h]) >= 5 and homes.get(h + 1)][0]
    chain, miss, bad = homes[H][:4], homes[H][4], homes[H + 1][0]
    wrap = homes[8191][:2] + homes[0][:1]
    miss_wrap = homes[0][1]
    taken = set(range(H - 1, H + 6)) | {8190, 8191, 0, 1, 2, 3}
    filler = [homes[h][0] for h in sorted(homes) if h not in taken and all(abs(h - t) > 8 for t in (H, 0, 8191))][5:5 + 12 * 40:40]
    a = Arrays(62, P)
    a.bad[bad] = 1
    a.kf([chain[0], filler[0], chain[1], bad, wrap[2], chain[2]] + filler[1:7] + [wrap[0], chain[3], wrap[1]] + filler[7:])
    a.kf(chain[::-1] + [bad, miss, wrap[1]] + filler)
    a.kf([wrap[0], miss_wrap, wrap[1], wrap[2]])
    c = case("cov_table_chains", [a], cov=[(0, 0, 8)])
    c["marks"] = dict(H=H, chain=chain, miss=miss, bad=bad, wrap=wrap, miss_wrap=miss_wrap)
    return c


def cov_table_full():
    """World 0: kf 0 has 4096 slots listing 4096 distinct good points (the table at load 0.5; indices drawn from 30 000, so that home
    cells collide); keyframe 1 observes all of them, keyframe 2 observes 4096 points kf 0 does not list. World 1: all 4096 slots of
    kf 0 list ONE point (the first slot observes it), keyframe 1 observes it once: weight 4096, 13 bits of the 16-bit count."""
    a = Arrays(63, 30000)
    pick = a.rng.permutation(30000)[:8192]
    a.kf(pick[:4096])
    a.kf(a.rng.permutation(pick[:4096]))
    a.kf(pick[4096:])
    b = Arrays(64, 16)
    b.kf([7] * 4096, [1] + [0] * 4095)
    b.kf([3, 7, -1])
    return case("cov_table_full", [a, b], cov=[(0, 0, 4), (1, 0, 4)])


WINDOW_E = {256: dict(sizes=(40, 60, 56, 50, 50), bad_at=255, null_at=254, twice=None),
            257: dict(sizes=(40, 60, 56, 50, 51), bad_at=100, null_at=255, twice=None),
            700: dict(sizes=(100, 156, 144, 150, 150), bad_at=255, null_at=256, twice=(5, 570))}


def window_E_world(E):
    """Six outside keyframes (0..5), then 1 + 4 local ones whose slot counts sum to E: tKFrame is keyframe 6 (its slots are the entries
    from 0 on), 7..10 are covisible. An entry lists a new point, except: entry `null_at` is a NULL slot, entry `bad_at` lists a bad
    point, entry twice[1] lists the point of entry twice[0] again, and every entry e with e % 7 == 3 relists a point of an earlier local
    keyframe (where there is one that this keyframe does not hold yet). Every third window point has an outside observer, every ninth two. Returns
    (builder, window spec)."""
    spec = WINDOW_E[E]
    b = World(70 + E)
    fixed = [b.kf(80) for _ in range(6)]
    local = [b.kf(n) for n in spec["sizes"]]
    e, at_entry, earlier, window_points = 0, {}, [], []
    for kf in local:
        here = []
        for _ in range(len(kf.mvMapPoints)):
            old = None
            if spec["twice"] and e == spec["twice"][1]:
                old = at_entry[spec["twice"][0]]
            elif e % 7 == 3 and earlier and e not in (spec["null_at"], spec["bad_at"]):
                old = earlier[(5 * e) % len(earlier)]
                old = None if old in kf.mvMapPoints else old
            if e == spec["null_at"]:
                b.slot(kf)
            elif e == spec["bad_at"]:
                b.point(kf).SetBadFlag()
            elif old is not None:
                b.see(kf, old)
            else:
                at_entry[e] = b.point(kf)
                here.append(at_entry[e])
                window_points.append(at_entry[e])
            e += 1
        earlier += here
    assert e == E
    for j, mp in enumerate(window_points[::3]):
        b.see(fixed[j % 6], mp)
    for j, mp in enumerate(window_points[::9]):                                      # (a second one for every ninth: never the same keyframe)
        b.see(fixed[(j + 3) % 6], mp)
    return b, (0, 6, [7, 8, 9, 10], -1, None, None, None)


def window_E(E):
    b, spec = window_E_world(E)
    return case(f"window_E_{E}", [b], windows=[spec], room=BIG_ROOM)


LONG_A, LONG_B = 7, 30


def window_long_segments():
    """60 outside keyframes (0..59), tKFrame 60 with 121 slots, 15 covisible keyframes of 9 slots. Window point 120 (the last slot of
    tKFrame) is observed by all 76 keyframes. Outside keyframe LONG_A has 130 slots and observes that point alone, at slot 129; LONG_B
    observes window point 101 at slot 3 and window point 11 at slot 70 (its place among the fixed keyframes is 11's, found by the
    wavefront's second trip); every other outside keyframe i observes window point 2 * (7 i mod 59) and point 120."""
    b = World(81)
    fixed = [b.kf(130 if i == LONG_A else 80 if i == LONG_B else 8) for i in range(60)]
    local = [b.kf(121)] + [b.kf(9) for _ in range(15)]
    pts = [b.point(local[0]) for _ in range(121)]
    for kf in local[1:]:
        for _ in range(8):
            b.point(kf)
        b.see(kf, pts[120])
    for i, f in enumerate(fixed):
        if i == LONG_A:
            b.link(f, 129, pts[120])
        elif i == LONG_B:
            b.link(f, 3, pts[101])
            b.link(f, 70, pts[11])
            b.link(f, 71, pts[120])
        else:
            b.see(f, pts[2 * ((7 * i) % 59)])
            b.see(f, pts[120])
    return case("window_long_segments", [b], windows=[(0, 60, list(range(61, 76)), -1, None, None, None)])


def window_table_chains():
    """Chosen indices, two sibling worlds with the same points. World 0: tKFrame 0 has 5 slots, the covisible keyframe 1 has 3: E = 8,
    T_bits = 4, 16 cells. Five of the seven window points have home cell 14 (the chain 14, 15, 0, 1, 2); point `twice` is listed by
    both keyframes; the outside keyframe 2 observes `miss`, not a window point, whose home is cell 15 (its probe walks 15, 0, 1, 2 and
    ends at the empty cell 3), and two window points. World 1: keyframe 1 has a fourth, NULL slot: E = 9, T_bits = 5, 32 cells — the same
    window out of another table."""
    P = 128
    chain = [p for p in range(P) if win_home(p, 4) == 14][:5]
    a, c = [[p for p in range(P) if win_home(p, 4) == h][0] for h in (6, 9)]
    miss = [p for p in range(P) if win_home(p, 4) == 15][0]
    twice = chain[1]
    worlds = []
    for extra in ([], [-1]):
        w = Arrays(65, P)
        w.kf(chain[:3] + [a, chain[3]])
        w.kf([chain[4], c, twice] + extra)
        w.kf([miss, chain[2], a, -1])
        worlds.append(w)
    out = case("window_table_chains", worlds, windows=[(0, 0, [1], -1, None, None, None), (1, 0, [1], -1, None, None, None)])
    out["marks"] = dict(chain=chain, others=[a, c], miss=miss, twice=twice)
    return out


def window_mixed_call():
    """One call of three very different windows: window_E_700's, a 5-entry window on a 6-keyframe map, and a window with 64 fixed
    keyframes on a 66-keyframe map (tKFrame 64: the second workgroup of the scan kernels holds the local keyframes)."""
    big, spec = window_E_world(700)
    tiny = World(82)
    k = [tiny.kf(6) for _ in range(4)] + [tiny.kf(2), tiny.kf(3)]
    tiny.share(k[4], k[5], 1)
    tiny.share(k[4], k[0], 1)
    tiny.share(k[5], k[1], 2)
    for kf in k[:4]:
        tiny.point(kf)
    wide = World(83)
    fixed = [wide.kf(2) for _ in range(64)]
    first, second = wide.kf(70), wide.kf(10)
    for f in fixed:
        wide.see(f, wide.point(first))
    wide.share(first, second, 5)
    return case("window_mixed_call", [big, tiny, wide], windows=[spec, (1, 4, [5], -1, None, None, None), (2, 64, [65], -1, None, None, None)], room=BIG_ROOM)


def commit_many_points(short):
    """window_E_700's window: every observation of every even window point, and of window points 255 and 256, is an outlier (they all go
    bad: more than 256 of them, in every 256-chunk of the window) — except the first window point from 512 on with three observations or
    more, which gets one outlier and stays good. bad_capacity: room for all, or short by one."""
    b, spec = window_E_world(700)
    win = BR.ba_window(b.world(), 6, [7, 8, 9, 10], -1)
    by_point = {}
    for j, i in enumerate(win["obs_point"]):
        by_point.setdefault(int(i), []).append((int(win["point_index"][i]), int(win["obs_slot"][j]) >> 32))
    stays = [i for i in range(512, win["n_points"]) if len(by_point[i]) >= 3][0]
    goes_bad = [i for i in range(win["n_points"]) if (i % 2 == 0 or i in (255, 256)) and i != stays]
    pairs = [pair for i in goes_bad for pair in by_point[i]] + by_point[stays][1:2]
    c = case("commit_many_points" + ("_bad_capacity_short_by_one" if short else ""), [b], windows=[spec], outliers={0: pairs}, room=BIG_ROOM,
             bad_capacity=len(goes_bad) - int(short))
    c["marks"] = dict(goes_bad=goes_bad, stays=stays)
    return c


def commit_overlap_beyond_256():
    """Two usable windows on one map, tKFrame 1 alone and tKFrame 2 alone, that share no keyframe and exactly one map point: listed by
    both keyframes and observed by nobody (an observer would be a fixed keyframe of both windows), at place 280 of the first window's
    points and 270 of the second's — the second workgroup of the claim kernels."""
    b = World(84)
    k = [b.kf(4), b.kf(300), b.kf(300)]
    b.point(k[0])
    for _ in range(280):
        b.point(k[1])
    for _ in range(270):
        b.point(k[2])
    shared = b.point(k[1], observe=False)
    b.see(k[2], shared, observe=False)
    c = case("commit_overlap_beyond_256", [b], windows=[(0, 1, [], -1, None, None, None), (0, 2, [], -1, None, None, None)], outliers={0: [], 1: []}, overlap=(0, 1))
    c["marks"] = dict(shared=shared.mlID)
    return c


def size_cases():
    return cached("ba_window_size", lambda: [cov_wide_keyframes(), cov_K(64), cov_K(65), cov_K(257), cov_table_chains(), cov_table_full(),
                                             window_E(256), window_E(257), window_E(700), window_long_segments(), window_table_chains(), window_mixed_call(),
                                             commit_many_points(False), commit_many_points(True), commit_overlap_beyond_256()])


def all_cases():
    return cached("ba_window_all", lambda: [cov_threshold(), cov_fallback_tie(), cov_nothing_shared(), cov_listed_twice_unobserved_and_bad(), cov_equal_weights(),
                                            window_basic(), window_origin(), window_short_capacities(), window_two_on_one_map_two_maps(), window_free_limit(),
                                            window_fixed_limit(64), window_fixed_limit(65)] + commit_cases() + [commit_overlap()])


def by_name(name):
    return [c for c in all_cases() + size_cases() if c["name"] == name][0]


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
                worlds[m], r = BR.ba_commit(worlds[m], win, win["T_c2w"], win["points"], e["flags"][i], c["bad_capacity"])
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
