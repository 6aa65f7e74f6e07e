"""The cases of dsdtm_slam_track_commit (include/dsdtm_amd_slam.h, rules T1-T4), shared by the CPU and the GPU half of its tests: small
maps built with the World builder of tests/ba_window_cases.py, one case per rule edge. A case is a dict: name, worlds (track_map_
restatement's), threshold, descs [(world, point, residual_norm)] in call order, bad_capacity (None: room for all), and `marks` (named
points, keyframes or slots the tests look at). expected(case) is the restatement's answer, computed once per session and never
changed. Test infrastructure only."""
import numpy as np

from dsdtm_amd import aftertrack_restatement as AR
from tests.ba_window_cases import World
from tests.track_map_cases import cached

THR = 0.0078125                         # an exact double; UP is the next one above it
UP = float(np.nextafter(THR, 1.0))
LOW, HIGH = THR / 2, THR * 2


def index_of(b, mp):
    return b.mps.index(mp)


def base(seed=41, n_kf=4, n_slots=12, shared=4):
    """n_kf keyframes; `shared` points observed by every keyframe, then each keyframe's own points up to half its slots."""
    b = World(seed)
    k = [b.kf(n_slots) for _ in range(n_kf)]
    for _ in range(shared):
        mp = b.point(k[0])
        for other in k[1:]:
            b.see(other, mp)
    for kf in k:
        for _ in range(n_slots // 2 - shared):
            b.point(kf)
    return b


def case(name, builders, descs, threshold=THR, bad_capacity=None, **marks):
    return dict(name=name, worlds=[b.world() for b in builders], threshold=threshold, descs=list(descs), bad_capacity=bad_capacity, marks=marks)


def three_below():                                          # 1
    b = base()
    for mp in b.mps[:3]:
        mp.mnFound = 7
    return case("three_matches_all_below_the_threshold", [b], [(0, [0, 1, 2], [LOW, 0.0, LOW])])


def threshold_edges():                                      # 2
    b = base(42)
    for mp in b.mps[:4]:
        mp.mnFound = 3
    return case("equal_is_kept_next_double_is_erased_nan_is_kept", [b], [(0, [0, 1, 2, 3], [THR, UP, float("nan"), float("inf")])])


def zero_to_bad():                                          # 3
    b = World(43)
    k = [b.kf(8) for _ in range(5)]
    for kf in k:
        b.point(kf)
    mp = b.point(k[0])
    b.see(k[1], mp)
    b.see(k[2], mp)
    b.see(k[3], mp, observe=False)                          # listed, not observing: the local-BA quirk
    mp.mnFound = 0
    return case("found_zero_goes_bad_three_observers_cleared_the_listed_slot_kept", [b], [(0, [index_of(b, mp), 0], [HIGH, LOW])], point=index_of(b, mp))


def found_five():                                           # 4
    b = base(44)
    b.mps[2].mnFound = 5
    return case("found_five_is_erased_back_to_five", [b], [(0, [2], [HIGH])])


def already_bad():                                          # 5
    b = base(45)
    b.mps[1].mnFound = 0
    b.mps[1].SetBadFlag()                                   # (the flag alone: its observing slots stay set)
    return case("a_point_bad_before_the_call_is_incremented_only", [b], [(0, [1, 5], [HIGH, HIGH])], point=1)


def shared_point(swap):                                     # 6
    b = base(46)
    b.mps[0].mnFound = b.mps[6].mnFound = 0
    b.mps[3].mnFound = 2
    first, second = (0, [0, 3, 6], [HIGH, LOW, LOW]), (0, [3, 0, 6], [HIGH, HIGH, HIGH])
    return case("two_descs_share_a_point_" + ("swapped" if swap else "in_order"), [b], [second, first] if swap else [first, second], point=0)


def two_maps():                                             # 7
    a, b = base(47), base(48, n_kf=3, n_slots=12)
    a.mps[1].mnFound = 0
    b.mps[2].mnFound = 0
    descs = [(0, [1, 4], [HIGH, LOW]), (1, [2, 0], [HIGH, HIGH]), (0, [4, 1, 8], [HIGH, HIGH, LOW]), (1, [], []), (1, [5], [LOW]), (0, [9], [HIGH]), (1, [2, 7], [HIGH, UP]),
             (0, [0, 1, 2, 3], [LOW, LOW, HIGH, HIGH])]
    return case("two_maps_eight_descs", [a, b], descs)


def lost_frame():                                           # 8
    return case("a_lost_frame_has_no_matches", [base(49)], [(0, [], [])])


def no_desc():
    return case("no_desc_at_all", [base(50)], [])


def one_match():                                            # 9
    b = base(51)
    b.mps[6].mnFound = 0
    return case("one_match", [b], [(0, [6], [HIGH])])


def full_house(short):
    b = World(52)
    k = [b.kf(48) for _ in range(6)]
    for kf in k:
        for _ in range(48):
            b.point(kf)
    for i, mp in enumerate(b.mps):
        mp.mnFound = 0 if i % 5 == 0 else 1 + i % 3
        if i % 7 == 0:
            b.link(k[(i // 48 + 1) % 6], 47 - (i % 48), mp)   # (a second observer, over the point that slot held: that point keeps its own slot's listing off)
    rng = np.random.default_rng(7)
    pts = rng.permutation(len(b.mps))[:256].tolist()
    norms = [HIGH if i % 2 == 0 else LOW for i in range(256)]
    n_bad = AR.track_commit(b.world(), THR, pts, norms)[1]["n_bad"]
    assert n_bad >= 8
    return case("256_matches" + ("_bad_capacity_short_by_one" if short else ""), [b], [(0, pts, norms)], bad_capacity=n_bad - 1 if short else None, n_bad=n_bad)


def wide_pool():                                            # 10
    """6 keyframes x 300 slots: 1800 slots, eight blocks of the cascade. The bad point's observers: the first slot of the pool, one in the
    middle, the last slot of the pool; a second bad point sits right at a block boundary (slots 255 and 256 of the pool)."""
    b = World(53)
    k = [b.kf(300) for _ in range(6)]
    mp = b.new_point(k[0], 0)
    b.link(k[3], 17, mp)
    b.link(k[5], 299, mp)
    edge = b.new_point(k[0], 255)
    other = b.new_point(k[0], 256)
    b.link(k[1], 0, other)
    for kf in k:
        for s in (5, 100, 298):
            b.new_point(kf, s)
    mp.mnFound = edge.mnFound = other.mnFound = 0
    pts = [index_of(b, other), index_of(b, mp), 7, index_of(b, edge)]
    return case("slot_pool_over_several_blocks", [b], [(0, pts, [HIGH, HIGH, LOW, HIGH])], point=index_of(b, mp))


# ---- dsdtm_slam_need_keyframes: trackers of tests/need_keyframe_cases.py turned into maps -------------------------------------------
def keyframe_world(c, holes=(), extra_kf=0, slots=None):
    """A map that holds the tracker `c` of need_keyframe_cases: the last keyframe's points, then the current frame's; keyframe 0 is the
    last keyframe (pose T_kf; its slots list its points in order, with a -1 slot in front of every list position in `holes` and one at
    the end — or, with `slots`, exactly that list: the position in c's kf list of the point each slot lists, ascending, or -1);
    keyframes 1 .. are the local keyframes, at [I | -centre] (so that Get_CameraCnt is the centre, exactly), then `extra_kf`
    more. Returns (world, tracker): tracker has T_cur_w, n_valid, cur_point, kf, local_kf and params."""
    kf_p, cur_p = np.asarray(c["kf_p"], np.float64).reshape(-1, 3), np.asarray(c["cur_p"], np.float64).reshape(-1, 3)
    nk, nc = len(kf_p), len(cur_p)
    flags = lambda b, n: np.zeros(n, np.uint8) if b is None else np.asarray(b, np.uint8).reshape(n)
    p_world = np.concatenate([kf_p, cur_p, np.zeros((1, 3))])              # (+ one point nobody names: a map has one at least)
    bad = np.concatenate([flags(c["kf_bad"], nk), flags(c["cur_bad"], nc), [0]]).astype(np.uint8)
    slots0 = []
    for i in range(nk):
        if i in holes:
            slots0.append(-1)
        slots0.append(i)
    slots0.append(-1)
    if slots is not None:
        slots0 = [int(p) for p in slots]
        assert [p for p in slots0 if p >= 0] == list(range(nk))
    lkf = np.asarray(c["lkf"], np.float64).reshape(-1, 3)
    poses = [np.asarray(c["T_kf"], np.float64).reshape(12)]
    for ctr in list(lkf) + [np.array([9.0, 9.0, 9.0])] * extra_kf:
        T = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
        T[[3, 7, 11]] = -ctr
        poses.append(T)
    slots = [np.array(slots0, np.int32)] + [np.array([nk + nc, -1], np.int32) for _ in poses[1:]]
    observes = [(s >= 0).astype(np.uint8) for s in slots]
    observes[0][::3] = 0                                                    # listed, not observing: still walked
    world = dict(p_world=p_world, bad=bad, found=np.ones(len(bad), np.int32), T_kf_w=np.array(poses).reshape(-1, 12), slots=slots, observes=observes,
                 px=[np.zeros((len(s), 2), np.float32) for s in slots], level=[np.zeros(len(s), np.int32) for s in slots],
                 bearing=[np.zeros((len(s), 3), np.float64) for s in slots])
    tracker = dict(T_cur_w=np.asarray(c["T_cur"], np.float64).reshape(12), n_valid=int(c["n_valid"]), cur_point=list(range(nk, nk + nc)), kf=0,
                   local_kf=list(range(1, 1 + len(lkf))), params=c["params"], cam=c["cam"])
    return world, tracker


ROUND = 256                             # the slots the gather kernel compacts per round


def long_keyframe(slots_of, n_slots):
    """A tracker of need_keyframe_cases whose last keyframe has n_slots slots: slots_of maps a slot to ("good", displacement in px) or
    ("bad", displacement); every other slot is -1. The current camera stands 8/512 beside the keyframe's and looks along +z, so a point
    (0, 0, z) is displaced by 8 / z px between the two images. Returns (case, slots)."""
    from dsdtm_amd.keyframe_decision import KeyframeParams
    from tests import need_keyframe_cases as NK
    kf_p, kf_bad, slots = [], [], []
    for s in range(n_slots):
        if s in slots_of:
            kind, px = slots_of[s]
            slots.append(len(kf_p))
            kf_p.append([0.0, 0.0, 8.0 / px])
            kf_bad.append(int(kind == "bad"))
        else:
            slots.append(-1)
    return NK.make(T_cur=NK.pose(8.0 / 512.0), kf_p=kf_p, kf_bad=kf_bad, params=KeyframeParams(min_trans=1.0)), slots


def long_keyframe_cases():
    """The last keyframes past one round of the gather's slot-order compaction. K2 samples the first 31 good points in slot order, so
    each world makes the verdict depend on the later rounds (tests/test_aftertrack_cpu.py holds them to that)."""
    out = {}
    out["kf_256_slots"] = {s: ("good", 8.0 + s) for s in range(256)}              # one full round, no second: sample 31 is slot 30
    w = {}                                                                          # slots 0..255: 30 good (15 at 8 px, 15 at 4096 px), 30 bad, holes
    for i in range(30):
        w[8 * i] = ("good", 8.0 if i % 2 == 0 else 4096.0)
        w[8 * i + 4] = ("bad", 64.0)
    w[256] = ("good", 128.0)                                                        # the 31st sample, and the median
    out["kf_257_slots_31st_sample_in_round_two"] = w
    w = {s: ("bad", 16.0 + s) for s in range(512) if s % 5 == 2 or s in (254, 257, 510)}      # (255, 256 and 511, 512 stay -1)
    w.update({520 + 2 * i: ("good", 32.0 + i) for i in range(40)})
    out["kf_600_slots_all_samples_from_round_three"] = w
    w = {3 + 20 * i: ("good", 8.0) for i in range(10)}                              # round one: 10 good, 40 bad
    w.update({4 + 6 * i: ("bad", 2048.0) for i in range(40)})
    for lane in range(64):                                                          # round two: wavefront 1 (5 good among bad), wavefront 3 (64 good)
        w[ROUND + 64 + lane] = ("good", 64.0 + lane) if lane in (3, 17, 31, 45, 63) else ("bad", 2048.0)
        w[ROUND + 192 + lane] = ("good", 256.0 + lane)
    out["kf_round_two_waves_1_and_3_only"] = w
    return {name: long_keyframe(w, {"kf_256_slots": 256, "kf_257_slots_31st_sample_in_round_two": 257, "kf_600_slots_all_samples_from_round_three": 600,
                                    "kf_round_two_waves_1_and_3_only": 512}[name]) for name, w in out.items()}


def keyframe_cases():
    """(name, world, tracker): one per deciding rule K1..K4; the 40-slot keyframe with -1 and bad slots mixed in (the 31-sample cut);
    bad points in the cur list; empty lists; 0 and 64 local keyframes; 4096 cur points; a point at z = 0 (undefined); and the long last
    keyframes of long_keyframe_cases (256, 257, 600 and 512 slots: one, two and three rounds of the gather's compaction)."""
    from tests import need_keyframe_cases as NK

    def make():
        out = []

        def add(name, c, **kw):
            out.append((name,) + keyframe_world(c, **kw))
        add("k1_decides", NK.EXACT["k1_low_edge"]())
        add("k2_decides", NK.EXACT["k2_above_threshold"](), holes=(0, 5, 6))
        add("k3_decides", NK.EXACT["k3_trans_equal"]())
        add("k4_decides", NK.EXACT["k4_equal"]())
        add("k4_fabs_quirk", NK.EXACT["k4_fabs_quirk"]())
        c = NK.EXACT["k2_31_stop"]()                                       # 40 points; bad ones and -1 slots in front of the cut
        c["kf_bad"] = np.array([1 if i in (2, 9, 30, 35) else 0 for i in range(40)], np.uint8)
        add("forty_slots_holes_and_bad_31_sample_cut", c, holes=(0, 1, 7, 20, 31, 39))
        add("small_then_huge_20", NK.EXACT["small_then_huge_20"](), holes=(3,))
        add("bad_points_in_the_cur_list", NK.random_case(5, 40, 35, 3, bad="some", fire=1))
        add("all_bad", NK.random_case(6, 20, 20, 2, bad="all"))
        add("empty_lists", NK.EXACT["empty_lists"]())
        add("no_local_keyframe", NK.random_case(7, 30, 33, 0, bad="none"), extra_kf=2)
        add("64_local_keyframes_last_fires", NK.random_case(8, 25, 40, 64, bad="some", fire=63))
        add("4096_cur_points", NK.random_case(9, 4096, 50, 4, bad="some", fire=2))
        add("a_point_at_z_0_is_undefined", NK.make(kf_p=[[0.0, 0.0, 1.0], [0.5, 0.5, 0.0], [0.0, 0.1, 1.0]], lkf=[[4.0, 3.2, 5.2]]), holes=(1,))
        for name, (c, slots) in long_keyframe_cases().items():
            add(name, c, slots=slots)
        return out
    return cached("aftertrack_keyframe_cases", make)


def gathered(world, tracker, gather=AR.gather_keyframe_desc):
    """The restated gather (or a deliberately wrong one, for the non-vacuity checks) as a tracker of need_keyframe_cases (what
    run_reference and desc_of take)."""
    g = gather(world, tracker["T_cur_w"], tracker["n_valid"], tracker["cur_point"], tracker["kf"], tracker["local_kf"])
    return dict(cam=tracker["cam"], T_cur=g["T_cur_w"].reshape(3, 4), T_kf=g["T_kf_w"].reshape(3, 4), n_valid=g["n_valid"], cur_p=g["cur_p_world"], cur_bad=g["cur_bad"],
                kf_p=g["kf_p_world"], kf_bad=g["kf_bad"], lkf=g["local_kf_centre"], params=tracker["params"])


def all_cases():
    return cached("aftertrack_all", lambda: [three_below(), threshold_edges(), zero_to_bad(), found_five(), already_bad(), shared_point(False), shared_point(True), two_maps(),
                                             lost_frame(), no_desc(), one_match(), full_house(False), full_house(True), wide_pool()])


def by_name(name):
    return [c for c in all_cases() if c["name"] == name][0]


def expected(c):
    """The restatement's answer: (worlds after, one result per desc)."""
    return cached(("aftertrack_expected", c["name"]), lambda: AR.track_commit_call(c["worlds"], c["threshold"], c["descs"], c["bad_capacity"]))


def flat(world, key, dtype):
    return np.concatenate([np.asarray(a, dtype).reshape(-1) for a in world[key]] + [np.zeros(0, dtype)])
