"""libdsdtm_amd_slam.so (include/dsdtm_amd_slam.h) without a GPU: the restatement of dsdtm_slam_track_commit
(dsdtm_amd/aftertrack_restatement.py) — the yardstick of the device entry, so it must not be its own — against the objects' own
bookkeeping and against track_commit_host through a compiled driver, what the cases are named for, the declaration / export / ctypes
mirror of the add-on library, and its host side as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer over the
fake HIP runtime (nothing is loaded into Python and nothing is preloaded)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from dsdtm_amd import aftertrack_restatement as AR
from dsdtm_amd import ba_window, capi, homography, local_map, motion, slam, track_map
from dsdtm_amd import keyframe_creation
from tests import aftertrack_cases as cases
from tests import fake_hip_build as fhb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_commit_equals_the_objects_bookkeeping():
    """IncreaseFound / EraseFound on copies of the objects as tracking.apply_tracked_frame walks them, with SetBadFlag as
    src/MapPoint.cpp:91-109 has it (the clearing of the observers done here, by hand, from the source: mObservations holds the observing
    slots only), desc after desc — against the restatement's world after every case with one map."""
    import copy
    from tests.track_map_cases import world_of
    from tests import ba_window_cases as bw
    b = cases.base(44)
    b.mps[0].mnFound = 0
    b.mps[5].mnFound = 0
    b.see(b.kfs[3], b.mps[5], observe=False)
    descs = [([0, 5, 2], [cases.HIGH, cases.HIGH, cases.LOW]), ([2, 0, 7], [cases.HIGH, cases.HIGH, cases.UP])]
    kfs, mps = copy.deepcopy((b.kfs, b.mps))
    want = [b.world()]
    for point, norm in descs:
        for p in point:
            mps[p].mnFound += 1
        for p, r in zip(point, norm):
            mp = mps[p]
            if r > cases.THR and not mp.IsBad():
                mp.mnFound -= 1
                if mp.mnFound <= 0:
                    mp.SetBadFlag()
                    for kf, s in list(mp._obs.items()):
                        kf.mvMapPoints[s] = None
                    mp._obs.clear()
        want, _ = AR.track_commit_call(want, cases.THR, [(0, point, norm)])
    bw.same_world(world_of(kfs, mps), want[0], "objects")
    assert want[0]["bad"][0] == 1 and want[0]["bad"][5] == 1 and 5 in want[0]["slots"][3] and 5 not in want[0]["slots"][0]


def test_the_cases_reach_what_they_are_named_for():
    by = {c["name"]: (c, cases.expected(c)) for c in cases.all_cases()}
    c, (after, r) = by["three_matches_all_below_the_threshold"]
    assert r[0]["n_erased"] == 0 and r[0]["found_after"] == [8, 8, 8] and np.array_equal(after[0]["bad"], c["worlds"][0]["bad"])
    c, (after, r) = by["equal_is_kept_next_double_is_erased_nan_is_kept"]
    assert r[0]["found_after"] == [4, 3, 4, 3] and r[0]["n_erased"] == 2 and r[0]["n_bad"] == 0 and cases.UP > cases.THR
    c, (after, r) = by["found_zero_goes_bad_three_observers_cleared_the_listed_slot_kept"]
    p = c["marks"]["point"]
    before = c["worlds"][0]
    assert [int(np.count_nonzero((s == p) & (o == 1))) for s, o in zip(before["slots"], before["observes"])] == [1, 1, 1, 0, 0]
    assert r[0]["bad_points"] == [p] and after[0]["found"][p] == 0 and after[0]["bad"][p] == 1
    assert [int(np.count_nonzero(s == p)) for s in after[0]["slots"]] == [0, 0, 0, 1, 0] and not any(o[s == p].any() for s, o in zip(after[0]["slots"], after[0]["observes"]))
    c, (after, r) = by["found_five_is_erased_back_to_five"]
    assert r[0]["found_after"] == [5] and r[0]["n_erased"] == 1 and r[0]["n_bad"] == 0
    c, (after, r) = by["a_point_bad_before_the_call_is_incremented_only"]
    assert r[0]["found_after"][0] == 1 and r[0]["n_erased"] == 1 and r[0]["n_bad"] == 0
    assert all(np.array_equal(a, b) for a, b in zip(after[0]["slots"], c["worlds"][0]["slots"])) and any((s == 1).any() for s in after[0]["slots"])
    (c0, (a0, r0)), (c1, (a1, r1)) = by["two_descs_share_a_point_in_order"], by["two_descs_share_a_point_swapped"]
    # in order: desc 0 turns point 0 bad, desc 1 increments it only (its two erases are points 3 and 6, and 6 stays good: 0 -> 1 -> 2 -> 1)
    assert r0[0]["bad_points"] == [0] and (r0[1]["n_erased"], r0[1]["n_bad"]) == (2, 0) and r0[1]["found_after"] == [3, 1, 1] and a0[0]["bad"][6] == 0
    # swapped: the three-match desc comes first and turns 0 AND 6 bad (0 -> 1 -> 0); the other one increments both only
    assert (r1[0]["n_erased"], r1[0]["bad_points"]) == (3, [0, 6]) and r1[0]["found_after"] == [2, 0, 0] and r1[1]["n_erased"] == 0 and r1[1]["found_after"] == [1, 3, 1]
    assert a1[0]["bad"][6] == 1 and not any((s == 6).any() for s in a1[0]["slots"]) and any((s == 6).any() for s in a0[0]["slots"])
    c, (after, r) = by["a_lost_frame_has_no_matches"]
    assert r == [dict(n_erased=0, n_bad=0, bad_points=[], found_after=[])] and np.array_equal(after[0]["found"], c["worlds"][0]["found"])
    c, (after, r) = by["256_matches_bad_capacity_short_by_one"]
    full = by["256_matches"][1][1][0]
    assert r[0]["overflow_bad"] == 1 and r[0]["n_bad"] == c["marks"]["n_bad"] and r[0]["bad_points"] == full["bad_points"][:-1] and len(c["descs"][0][1]) == 256
    c, (after, r) = by["slot_pool_over_several_blocks"]
    S = cases.flat(c["worlds"][0], "slots", np.int32)
    assert len(S) == 1800 and S[0] == c["marks"]["point"] and S[-1] == c["marks"]["point"] and r[0]["n_bad"] == 3
    assert not (cases.flat(after[0], "slots", np.int32) == c["marks"]["point"]).any() and cases.flat(after[0], "slots", np.int32)[[0, 255, 256, 300, 1799]].tolist() == [-1] * 5


def test_the_restatement_refuses_what_the_entry_refuses():
    w = cases.base().world()
    for point, norm, thr, what in (([0, 1, 0], [0, 0, 0], cases.THR, "twice"), ([0, len(w["bad"])], [0, 0], cases.THR, "outside"), ([-1], [0], cases.THR, "outside"),
                                   ([0], [0], float("nan"), "finite"), ([0], [0], float("inf"), "finite"), (list(range(20)) * 13, [0] * 260, cases.THR, "n_matches")):
        with pytest.raises(ValueError, match=what):
            AR.track_commit_call([w], thr, [(0, point, norm)])
    with pytest.raises(ValueError, match="bad_capacity"):
        AR.track_commit_call([w], cases.THR, [], -1)


def test_host_function_agrees_with_the_restatement(tmp_path):
    """track_commit_host (plain C++, no device call) through the compiled driver on every case: the counts, the bad lists, found_after
    and the whole map after the descs, byte for byte. One job per map of a case; its descs run in call order."""
    jobs = []
    for c in cases.all_cases():
        after, results = cases.expected(c) if c["bad_capacity"] is None else AR.track_commit_call(c["worlds"], c["threshold"], c["descs"])
        for m, world in enumerate(c["worlds"]):
            jobs.append((c["name"], world, c["threshold"], [(d, r) for d, r in zip(c["descs"], results) if d[0] == m], after[m]))
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("i", len(jobs)))
        for name, world, thr, descs, _ in jobs:
            f.write(struct.pack("2i", len(world["bad"]), len(world["slots"])))
            f.write(np.ascontiguousarray(world["found"], np.int32).tobytes() + np.ascontiguousarray(world["bad"], np.uint8).tobytes())
            f.write(np.array([len(x) for x in world["slots"]], np.int32).tobytes())
            f.write(cases.flat(world, "slots", np.int32).tobytes() + cases.flat(world, "observes", np.uint8).tobytes())
            f.write(struct.pack("d", thr) + struct.pack("i", len(descs)))
            for (_, point, norm), _ in descs:
                f.write(struct.pack("i", len(point)) + np.asarray(point, np.int32).tobytes() + np.asarray(norm, np.float64).tobytes())
    exe = str(tmp_path / "aftertrack_driver")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "aftertrack_host", "driver.cpp")], check=True)
    subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], check=True)
    buf, at = open(tmp_path / "answers.bin", "rb").read(), 0

    def take(dt, n):
        nonlocal at
        a = np.frombuffer(buf, dt, n, at).copy()
        at += a.nbytes
        return a
    for name, world, _, descs, after in jobs:
        for (_, point, _), r in descs:
            n_erased, n_bad = (int(v) for v in take(np.int32, 2))
            assert (n_erased, n_bad) == (r["n_erased"], r["n_bad"]), name
            assert take(np.int32, n_bad).tolist() == r["bad_points"] and take(np.int32, len(point)).tolist() == r["found_after"], name
        P, S = len(after["bad"]), sum(len(x) for x in after["slots"])
        assert np.array_equal(take(np.int32, P), after["found"]) and np.array_equal(take(np.uint8, P), after["bad"]), name
        assert np.array_equal(take(np.int32, S), cases.flat(after, "slots", np.int32)) and np.array_equal(take(np.uint8, S), cases.flat(after, "observes", np.uint8)), name
    assert at == len(buf)


def test_gathered_keyframe_lists_agree_and_decide_as_the_tracker_they_were_made_from(tmp_path):
    """gather_keyframe_desc_host (plain C++, -ffp-contract=off) through the compiled driver against the restated gather on every
    keyframe case: counts, poses, both point lists with their flags and the camera centres, bit for bit. And the restated gather is
    what the case was built from — the lists of the need_keyframe_cases tracker, the centres exactly — so keyframe_decision decides on
    it as on the tracker."""
    from tests import need_keyframe_cases as NK
    kcs = cases.keyframe_cases()
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("i", len(kcs)))
        for name, world, t in kcs:
            f.write(struct.pack("2i", len(world["bad"]), len(world["slots"])))
            f.write(np.ascontiguousarray(world["p_world"], np.float64).tobytes() + np.ascontiguousarray(world["bad"], np.uint8).tobytes())
            f.write(np.ascontiguousarray(world["T_kf_w"], np.float64).tobytes() + np.array([len(x) for x in world["slots"]], np.int32).tobytes())
            f.write(cases.flat(world, "slots", np.int32).tobytes())
            f.write(np.asarray(t["T_cur_w"], np.float64).tobytes() + struct.pack("4i", t["n_valid"], len(t["cur_point"]), t["kf"], len(t["local_kf"])))
            f.write(np.asarray(t["cur_point"], np.int32).tobytes() + np.asarray(t["local_kf"], np.int32).tobytes())
    exe = str(tmp_path / "gather_driver")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "aftertrack_host", "gather_driver.cpp")], check=True)
    subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], check=True)
    buf, at = open(tmp_path / "answers.bin", "rb").read(), 0

    def take(dt, n):
        nonlocal at
        a = np.frombuffer(buf, dt, n, at).copy()
        at += a.nbytes
        return a
    from tests.track_map_cases import same_bits
    for name, world, t in kcs:
        g = AR.gather_keyframe_desc(world, t["T_cur_w"], t["n_valid"], t["cur_point"], t["kf"], t["local_kf"])
        n_valid, nc, nk, nl = (int(v) for v in take(np.int32, 4))
        assert (n_valid, nc, nk, nl) == (g["n_valid"], len(g["cur_bad"]), len(g["kf_bad"]), len(g["local_kf_centre"])), name
        assert same_bits(take(np.float64, 12), g["T_cur_w"]) and same_bits(take(np.float64, 12), g["T_kf_w"]), name
        assert same_bits(take(np.float64, 3 * nc), g["cur_p_world"].reshape(-1)) and np.array_equal(take(np.uint8, nc), g["cur_bad"]), name
        assert same_bits(take(np.float64, 3 * nk), g["kf_p_world"].reshape(-1)) and np.array_equal(take(np.uint8, nk), g["kf_bad"]), name
        assert same_bits(take(np.float64, 3 * nl), g["local_kf_centre"].reshape(-1)), name
    assert at == len(buf)
    by = {name: (world, t) for name, world, t in kcs}
    src = {"k1_decides": NK.EXACT["k1_low_edge"](), "k2_decides": NK.EXACT["k2_above_threshold"](), "k3_decides": NK.EXACT["k3_trans_equal"](),
           "k4_decides": NK.EXACT["k4_equal"](), "k4_fabs_quirk": NK.EXACT["k4_fabs_quirk"](), "64_local_keyframes_last_fires": NK.random_case(8, 25, 40, 64, bad="some", fire=63)}
    want_reason = {"k1_decides": 1, "k2_decides": 2, "k3_decides": 3, "k4_decides": 4, "k4_fabs_quirk": 0, "64_local_keyframes_last_fires": None}
    for name, c in src.items():
        got = cases.gathered(*by[name])
        assert same_bits(got["kf_p"], c["kf_p"]) and same_bits(got["cur_p"], c["cur_p"]) and same_bits(got["lkf"], c["lkf"]), name
        r = NK.run_reference(got)
        assert r == NK.run_reference(c) and (want_reason[name] is None or r["reason"] == want_reason[name]), (name, r)
    assert NK.run_reference(cases.gathered(*by["64_local_keyframes_last_fires"]))["svo_kf"] == 63
    r = NK.run_reference(cases.gathered(*by["forty_slots_holes_and_bad_31_sample_cut"]))
    world, t = by["forty_slots_holes_and_bad_31_sample_cut"]
    assert r["n_px"] == 31 and len(world["slots"][0]) == 47 and int(np.count_nonzero(world["slots"][0] < 0)) == 7 and int(world["bad"][:40].sum()) == 4
    assert NK.run_reference(cases.gathered(*by["a_point_at_z_0_is_undefined"]))["undefined"] == 1
    assert NK.run_reference(cases.gathered(*by["empty_lists"]))["n_px"] == 0 and len(by["4096_cur_points"][1]["cur_point"]) == 4096
    for bad_call, what in ((dict(kf=99), "kf is not"), (dict(cur_point=[10 ** 6]), "cur_point"), (dict(local_kf=[99]), "local_kf"), (dict(T_cur_w=np.full(12, np.nan)), "finite"),
                           (dict(cur_point=[0] * 4097), "n_cur_points"), (dict(local_kf=[0] * 65), "n_local_kf")):
        world, t = by["k4_decides"]
        q = dict(t, **bad_call)
        with pytest.raises(ValueError, match=what):
            AR.gather_keyframe_desc(world, q["T_cur_w"], q["n_valid"], q["cur_point"], q["kf"], q["local_kf"])


def _round_lists(world, kf):
    """The restated gather of each 256-slot round of keyframe kf alone: [(kf_p_world, kf_bad)]."""
    out = []
    for s0 in range(0, len(world["slots"][kf]), cases.ROUND):
        one = dict(world, slots=[s[s0:s0 + cases.ROUND] if k == kf else s for k, s in enumerate(world["slots"])])
        g = AR.gather_keyframe_desc(one, np.zeros(12), 0, [], kf, [])
        out.append((g["kf_p_world"], g["kf_bad"]))
    return out


def gather_base_not_carried(world, T_cur_w, n_valid, cur_point, kf, local_kf):
    """A deliberately WRONG gather: every round compacts from 0, so a round overwrites the front of the list the earlier rounds left
    (the list is as long as the longest round's)."""
    g = AR.gather_keyframe_desc(world, T_cur_w, n_valid, cur_point, kf, local_kf)
    rounds = _round_lists(world, kf)
    n = max([len(b) for _, b in rounds] + [0])
    p, bad = np.zeros((n, 3)), np.zeros(n, np.uint8)
    for rp, rb in rounds:
        p[:len(rb)], bad[:len(rb)] = rp, rb
    return dict(g, kf_p_world=p, kf_bad=bad)


def gather_later_rounds_dropped(world, T_cur_w, n_valid, cur_point, kf, local_kf):
    """A deliberately WRONG gather: the rounds after the first are dropped."""
    g = AR.gather_keyframe_desc(world, T_cur_w, n_valid, cur_point, kf, local_kf)
    rounds = _round_lists(world, kf)
    return dict(g, kf_p_world=rounds[0][0], kf_bad=rounds[0][1]) if rounds else g


def test_the_long_keyframes_verdicts_depend_on_the_later_rounds_of_the_gather():
    """The gather is visible only through the verdict, and K2 stops after 31 samples: each long last keyframe is arranged so that a
    gather that loses the running base, or the rounds after the first, gives OTHER reference verdict bytes — except kf_256_slots, which
    has no second round (there all three agree). WHAT CANNOT DIFFER: on kf_600_slots_all_samples_from_round_three the base-not-carried
    gather gives the SAME verdict as the faithful one, whatever it leaves behind the overwritten front: rounds one and two hold no good
    point, so the first 31 good points of either list are round three's, in the same order. That world is held to the lost base by
    its gathered list (which differs) and to the dropped rounds by its verdict; the two worlds with good points in front of the
    later rounds show the lost base in the verdict."""
    from tests import need_keyframe_cases as NK
    by = {name: (world, t) for name, world, t in cases.keyframe_cases()}

    def verdict(world, t, gather):
        r = NK.run_reference(cases.gathered(world, t, gather))
        return struct.pack("7i5d", *[r[k] for k in NK.INT_FIELDS + NK.FLOAT_FIELDS]), r
    want_n_px = {"kf_256_slots": 31, "kf_257_slots_31st_sample_in_round_two": 31, "kf_600_slots_all_samples_from_round_three": 31, "kf_round_two_waves_1_and_3_only": 31}
    for name in cases.long_keyframe_cases():
        world, t = by[name]
        good, r = verdict(world, t, AR.gather_keyframe_desc)
        no_base, dropped = verdict(world, t, gather_base_not_carried)[0], verdict(world, t, gather_later_rounds_dropped)[0]
        assert r["n_px"] == want_n_px[name] and r["undefined"] == 0, (name, r)
        if name == "kf_256_slots":
            assert no_base == good and dropped == good
            continue
        assert dropped != good, name
        if name == "kf_600_slots_all_samples_from_round_three":
            a, b = cases.gathered(world, t), cases.gathered(world, t, gather_base_not_carried)
            assert no_base == good and (len(a["kf_bad"]) != len(b["kf_bad"]) or a["kf_p"].tobytes() != b["kf_p"].tobytes())
        else:
            assert no_base != good, name
    # and what each world is named for
    slots = {name: by[name][0]["slots"][0] for name in cases.long_keyframe_cases()}
    bad = {name: by[name][0]["bad"] for name in slots}
    good_slots = lambda name: [s for s, p in enumerate(slots[name]) if p >= 0 and not bad[name][p]]
    assert len(slots["kf_256_slots"]) == 256 and (slots["kf_256_slots"] >= 0).all() and good_slots("kf_256_slots")[30] == 30
    g = good_slots("kf_257_slots_31st_sample_in_round_two")
    r = verdict(*by["kf_257_slots_31st_sample_in_round_two"], AR.gather_keyframe_desc)[1]
    assert len(slots["kf_257_slots_31st_sample_in_round_two"]) == 257 and len(g) == 31 and g[30] == 256 and r["median_px"] == 128.0
    assert sorted(r["px_dist"]) == [8.0] * 15 + [128.0] + [4096.0] * 15 and (slots["kf_257_slots_31st_sample_in_round_two"][:256] < 0).any()
    assert int(bad["kf_257_slots_31st_sample_in_round_two"][slots["kf_257_slots_31st_sample_in_round_two"][:256][slots["kf_257_slots_31st_sample_in_round_two"][:256] >= 0]].sum()) == 30
    s, g = slots["kf_600_slots_all_samples_from_round_three"], good_slots("kf_600_slots_all_samples_from_round_three")
    assert len(s) == 600 and len(g) == 40 and min(g) >= 512 and (s[[255, 256, 511, 512]] == -1).all() and (s[[254, 257, 510]] >= 0).all()
    assert len(set(verdict(*by["kf_600_slots_all_samples_from_round_three"], AR.gather_keyframe_desc)[1]["px_dist"])) == 31
    s, g = slots["kf_round_two_waves_1_and_3_only"], good_slots("kf_round_two_waves_1_and_3_only")
    in_round_two = np.flatnonzero(s[256:] >= 0)
    assert len(s) == 512 and set((in_round_two // 64).tolist()) == {1, 3} and len(in_round_two) == 128 and 0 < int((s[:256] >= 0).sum()) < 256
    assert [x for x in g[:31] if x < 256] == g[:10] and [x for x in g[:31] if 320 <= x < 384] == g[10:15] and min(g[15:31]) >= 448      # samples from both wavefronts


def test_example_and_adapter_compile():
    """example_aftertrack.cpp uses Tracking::CommitTrackedFrameOnDevice of dsdtm_slam_host.hpp and track_commit_host: the compiler sees
    them here."""
    path = os.path.join(ROOT, "dsdtm_amd", "host", "example_aftertrack.cpp")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", path], check=True)
    src = open(path).read()
    assert "CommitTrackedFrameOnDevice(" in src and "track_commit_host(" in src and "NeedKeyframeOnMap(" in src and "gather_keyframe_desc_host(" in src


def _lib_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_declared_exported_and_mirrored(tmp_path):
    """The library exports exactly what its header declares — the map's 11 entries, the mapping thread's 3, the commit and the keyframe decision — and reads no
    environment; the ctypes mirror has the header's layouts and limits; the eight older libraries export what their bindings list, the
    mapping library its 14 symbols from the body now compiled twice."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_slam.h")).read()
    assert re.search(r"#define DSDTM_SLAM_MAX_MATCHES %d\b" % AR.MAX_MATCHES, hdr) and slam.MAX_MATCHES == AR.MAX_MATCHES
    assert AR.MAX_DESCS == slam.MAX_DESCS == local_map.MAX_DESCS
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", code))
    assert declared == set(slam.SYMBOLS) and len(slam.SYMBOLS) == 16
    assert _lib_symbols(slam.lib_path()) == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", slam.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    lib = slam.load()
    for sym in slam.SYMBOLS:
        decl = re.search(r"\b%s\(([^;]*?)\);" % sym, code, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == len(getattr(lib, sym).argtypes), sym
    assert _lib_symbols(ba_window.lib_path()) == set(ba_window.SYMBOLS) and len(ba_window.SYMBOLS) == 14
    assert _lib_symbols(track_map.lib_path()) == set(track_map.SYMBOLS) and len(track_map.SYMBOLS) == 11
    assert _lib_symbols(local_map.lib_path()) == set(local_map.SYMBOLS) and _lib_symbols(capi.lib_path()) == set(capi.EXPORTED_SYMBOLS) and len(capi.EXPORTED_SYMBOLS) == 38
    assert _lib_symbols(motion.lib_path()) == set(motion.SYMBOLS) and _lib_symbols(homography.lib_path()) == set(homography.SYMBOLS)
    assert _lib_symbols(keyframe_creation.lib_path()) == set(keyframe_creation.SYMBOLS)
    kf_hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsdtm_amd_keyframe.h")).read(), flags=re.S)
    assert _lib_symbols(os.path.join(ROOT, "dsdtm_amd", "csrc", "libdsdtm_amd_keyframe.so")) == set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", kf_hdr))
    structs = [("dsdtm_slam_commit_desc", slam.CommitDesc), ("dsdtm_slam_commit_result", slam.CommitResult), ("dsdtm_slam_keyframe_desc", slam.KeyframeDesc)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_slam.h"', 'int main(void) {']
    for cname, ct in structs:
        src.append(f'  printf("%zu", sizeof({cname}));')
        src += [f'  printf(" %zu", offsetof({cname}, {f}));' for f, _ in ct._fields_]
        src.append('  printf("\\n");')
    src += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    lines = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for (cname, ct), line in zip(structs, lines):
        assert [int(v) for v in line.split()] == [C.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_], cname


def test_header_states_the_rules_and_the_quirks():
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_slam.h")).read()
    for needle in ("src/Feature_alignment.cpp:106", "src/Optimizer.cpp:81-94", "src/Optimizer.cpp:84-92", "src/MapPoint.cpp:191-197", "src/MapPoint.cpp:98-105",
                   "src/Optimizer.cpp:22-24", "src/Tracking.cpp:294-297", "T1 ", "T2 ", "T3 ", "T4 ", "a NaN norm erases\n *   nothing", "whether p is bad or not",
                   "without observing it keeps it", "bad before the call", "remain for callers who want one stage alone", "THE SAME\n *   POINT TWICE IN ONE DESC", "src/Tracking.cpp:347-410", "WHY THE SLOT WALK IS THE WALK OVER mvFeatures[i]->Mpt",
                   "c_i = -((R_0i * t_0 + R_1i * t_1) + R_2i * t_2)", "no fused multiply-add", "byte-equal to dsdtm_need_keyframes", "dsdtm_slam_points_write refuses"):
        assert needle in hdr, needle


def test_slam_host_side_under_address_and_ub_sanitizers(tmp_path):
    """dsdtm_amd/csrc/slam_api.cpp as a stand-alone program (tests/fake_hip_slam/driver.cpp, its own main) built with
    -fsanitize=address,undefined and executed: every refusal with the map read back unchanged, each HIP call failing in turn with the
    map's bookkeeping unchanged and the context usable, descs grouped by map, the staging blocks growing — for BOTH new entries: the
    gather of dsdtm_slam_need_keyframes reaches the (faked) decision kernel whole, its refusals leave the verdicts untouched."""
    here = os.path.join(fhb.ROOT, "tests", "fake_hip_slam")
    others = [os.path.join(fhb.ROOT, "tests", d) for d in ("fake_hip_mapping", "fake_hip_trackmap", "fake_hip_localmap", "fake_hip_keyframe")]
    exe = fhb.build_driver(tmp_path, "asan", [os.path.join(here, "driver.cpp"), os.path.join(here, "fake_slam.cpp"), os.path.join(others[0], "fake_mapping.cpp"),
                                              os.path.join(others[1], "fake_trackmap.cpp"), os.path.join(others[2], "fake_localmap.cpp"), os.path.join(others[3], "fake_keyframe.cpp")], ["slam_api.cpp"],
                           include_dirs=[here, *others])
    r, lines = fhb.run_driver(exe, "asan")
    assert lines == ["ok commits_and_growth", "ok validation", "ok hip_failures", "ok keyframes_and_validation", "ok keyframe_hip_failures", "ok create_failures"], (lines, r.stderr[-3000:])
