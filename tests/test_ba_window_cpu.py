"""libdsdtm_amd_mapping.so (include/dsdtm_amd_mapping.h) without a GPU: the restatement (dsdtm_amd/ba_window_restatement.py) — the
yardstick of the device entries, so it must not be its own — against the object-walking adapter Optimizer.LocalBundleAdjustment and the
objects' own bookkeeping, what the cases are named for, and the declaration / export / ctypes mirror of the add-on library."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from dsdtm_amd import ba_window, capi, homography, local_map, motion, track_map
from dsdtm_amd import ba_window_restatement as BR
from dsdtm_amd.optimizer import Optimizer
from tests import ba_window_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERY = cases.all_cases() + cases.size_cases()
WINDOWED = [c for c in EVERY if c["windows"] and c["objects"][0][0] is not None]      # (a world of plain arrays has no objects to walk)


@pytest.mark.parametrize("c", WINDOWED, ids=lambda c: c["name"])
def test_restated_window_equals_the_object_walking_adapter(c):
    """Optimizer.LocalBundleAdjustment (dsdtm_amd/optimizer.py) with a stub solve, on fresh copies of the objects (the window is what the
    reference builds the FIRST time it is asked), against ba_window with origin_kf = 0: the adapter knows the origin as mlId == 0, so
    every case is restated with that origin here, whatever origin the case itself asks for (those are held to the rules by the tests
    below). Local keyframes, points, constants and every point's columns are equal. WHERE THEY CANNOT AGREE: the adapter walks
    mObservations in the dict's insertion order, the window rules in ascending keyframe index (this project's definition of the
    reference's pointer order) — so the fixed keyframes are compared as a set with their poses and constants, and each point's
    observations as a set of (map keyframe, bearing, level) rows. The columns of a window that is NOT usable are not compared (the
    restatement returns none): the over-limit and capacity cases are held to the adapter by their counts alone."""
    for w, kf, cov, _, _, _, _ in c["windows"]:
        kfs, mps = copy.deepcopy(c["objects"][w])
        kfs[kf].mOrderedCovGraph = [(0, kfs[k]) for k in cov]
        seen = {}

        def solve(T, const, X, okf, opt, bearing, level, thresh):
            seen.update(T=T.reshape(-1, 12).copy(), const=const.copy(), X=X.reshape(-1, 3).copy(), okf=okf.copy(), opt=opt.copy(), bearing=bearing.copy(), level=level.copy())
            return np.zeros(len(okf), np.uint8), {}
        Optimizer.LocalBundleAdjustment(kfs[kf], solve=solve)
        want = BR.ba_window(c["worlds"][w], kf, cov, 0)
        nl = want["n_local"]
        assert len(seen["T"]) == nl + want["n_fixed"] and len(seen["X"]) == want["n_points"] and len(seen["okf"]) == want["n_obs"]
        if not want["usable"]:
            continue
        assert cases.same_bits(seen["T"][:nl], want["T_c2w"][:nl]) and np.array_equal(seen["const"][:nl], want["kf_constant"][:nl])
        assert cases.same_bits(seen["X"], want["points"]) and np.array_equal(seen["opt"], want["obs_point"])
        pose_of = lambda T, const: sorted((t.tobytes(), int(k)) for t, k in zip(T, const))
        assert pose_of(seen["T"][nl:], seen["const"][nl:]) == pose_of(want["T_c2w"][nl:], want["kf_constant"][nl:])
        rows = lambda T, okf, opt, b, lv: sorted((int(p), T[k].tobytes(), b[j].tobytes(), int(lv[j])) for j, (k, p) in enumerate(zip(okf, opt)))
        assert rows(seen["T"], seen["okf"], seen["opt"], seen["bearing"], seen["level"]) == rows(want["T_c2w"], want["obs_kf"], want["obs_point"], want["obs_bearing"], want["obs_level"])


def test_restated_commit_equals_the_objects_bookkeeping():
    """The outlier pass on the objects — MapPoint::Erase_Observation, then KeyFrame::Erase_MapPointMatch, with SetBadFlag as
    src/MapPoint.cpp:91-109 has it (mapping.MapPoint.SetBadFlag only sets the flag, so the clearing of the observers is done here, by
    hand, from the source) — against ba_commit on every commit case."""
    for c in [c for c in EVERY if c["outliers"] is not None and not c["overlap"]]:
        e = cases.expected(c)
        kfs, mps = copy.deepcopy(c["objects"][0])
        win = e["windows"][0]
        n_out = 0
        for j in np.flatnonzero(e["flags"][0]):
            mp, kf = mps[win["point_index"][win["obs_point"][j]]], kfs[int(win["obs_slot"][j]) >> 32]
            n_out += 1
            was_bad = mp.IsBad()
            left = mp.Get_Observations() if not was_bad else {}
            mp.Erase_Observation(kf)
            if mp.IsBad() and not was_bad:                  # SetBadFlag: mObservations.clear(), Erase_MapPointMatch(index) in every observer left
                for k2, s2 in left.items():
                    if k2 is not kf:
                        k2.mvMapPoints[s2] = None
                mp._obs.clear()
            kf.Erase_MapPointMatch(mp)
        after = cases.world_of(kfs, mps)
        cases.same_world(after, e["worlds_after"][0], c["name"])
        was_bad = {p for p, mp in enumerate(c["objects"][0][1]) if mp.IsBad()}
        went_bad = [p for p, mp in enumerate(mps) if mp.IsBad() and p not in was_bad]      # (bad before the commit: a size world's bad entry)
        full = e["commits"][0]["bad_points"] if c["bad_capacity"] is None else BR.ba_commit(c["worlds"][0], win, win["T_c2w"], win["points"], e["flags"][0])[1]["bad_points"]
        assert n_out == e["commits"][0]["n_outliers"] and went_bad == full and len(full) == e["commits"][0]["n_bad"]


def test_the_cases_reach_what_they_are_named_for():
    by = {c["name"]: cases.expected(c) for c in cases.all_cases()}
    assert by["cov_weight_15_is_out_16_is_in"]["cov"][0] == dict(n_cov=1, n_connected=2, overflow=0, cov_kf=[2], cov_weight=[16])
    assert by["cov_none_above_15_tie_lowest_index"]["cov"][0]["cov_kf"] == [1] and by["cov_none_above_15_tie_lowest_index"]["cov"][0]["cov_weight"] == [5]
    assert by["cov_no_shared_point"]["cov"][0]["n_cov"] == 0 and by["cov_no_shared_point"]["cov"][0]["n_connected"] == 0
    r = by["cov_listed_twice_listed_unobserved_bad_point"]["cov"][0]
    assert r["cov_kf"] == [1] and r["cov_weight"] == [4] and r["n_connected"] == 3      # 3 shared + the second listing; kf 2: 1; kf 3: 4 - the bad one
    r = by["cov_equal_weights_sort_by_index_and_overflow"]["cov"]
    assert r[0]["cov_kf"] == [1, 2, 3] and r[1]["overflow"] == 1 and r[1]["cov_kf"] == [1, 2] and r[2]["n_cov"] == 3
    w = by["window_first_occurrence_fixed_order_listed_unobserved"]["windows"][0]
    assert w["kf_index"].tolist() == [5, 3, 4, 2, 1, 0] and w["kf_constant"].tolist() == [0, 0, 0, 1, 1, 1] and len(set(w["point_index"].tolist())) == w["n_points"]
    w = by["window_kf_is_origin_no_points_and_origin_in_cov_is_constant"]["windows"]
    assert (w[0]["n_points"], w[0]["usable"], w[0]["kf_constant"].tolist()) == (0, 1, [1, 0, 0]) and w[1]["kf_constant"].tolist()[:3] == [0, 1, 0]
    assert w[2]["n_local"] == 1 and w[2]["usable"] == 1 and w[3]["usable"] == 0 and not any(w[3][f] for f in BR.FLAGS)
    flags = [[f for f in BR.FLAGS if x[f]] for x in by["window_each_capacity_short_by_one"]["windows"]]
    assert flags == [["over_keyframe_capacity"], ["over_point_capacity"], ["over_observation_capacity"], []]
    w = by["window_16_and_17_free_keyframes"]["windows"]
    assert [x["usable"] for x in w] == [1, 0, 1] and w[1]["over_free_kf"] == 1 and w[2]["n_local"] == 17 and w[2]["kf_constant"][1] == 1
    assert by["window_64_fixed_keyframes"]["windows"][0]["usable"] == 1 and by["window_64_fixed_keyframes"]["windows"][0]["n_fixed"] == 64
    assert by["window_65_fixed_keyframes"]["windows"][0]["over_const_kf"] == 1 and by["window_65_fixed_keyframes"]["windows"][0]["usable"] == 0
    commits = {n[len("commit_"):]: e["commits"][0] for n, e in by.items() if n.startswith("commit_") and e.get("commits") and e["commits"][0]}
    assert (commits["one_of_three_point_stays_good"]["n_outliers"], commits["one_of_three_point_stays_good"]["n_bad"]) == (1, 0)
    assert commits["three_of_three_third_changes_nothing"]["n_outliers"] == 3 and commits["three_of_three_third_changes_nothing"]["n_bad"] == 1
    assert commits["single_observation_is_an_outlier"]["n_bad"] == 1 and commits["all_of_them_together"]["n_bad"] == 4
    assert by["commit_two_overlapping_windows_refused"]["overlap"] == (0, 1)
    # one of two: the other slot is nulled, the outlier's slot is kept (the quirk of include/dsdtm_amd_trackmap.h)
    c = cases.by_name("commit_one_of_two_point_goes_bad")
    (p, k), after = c["outliers"][0][0], by[c["name"]]["worlds_after"][0]
    assert p in after["slots"][k] and p not in after["slots"][3] and after["bad"][p] == 1 and not after["observes"][k][list(after["slots"][k]).index(p)]


def test_the_size_cases_cross_what_they_are_named_for():
    """Every size world against the boundary its name claims, on the restatement's answer and on the Python model of the two tables
    (cases.probe_table with the restated hashes): a size world that stops crossing its boundary fails HERE, not vacuously on the GPU."""
    size = {c["name"]: c for c in cases.size_cases()}
    by = {n: cases.expected(c) for n, c in size.items()}
    W = lambda name, m=0: size[name]["worlds"][m]
    n_slots = lambda name, m=0: [len(s) for s in W(name, m)["slots"]]
    # -- covisibility
    w = W("cov_wide_keyframes")
    assert n_slots("cov_wide_keyframes")[:4] == [300, 64, 65, 130] and w["slots"][0][10] == w["slots"][0][270] >= 0
    for k, s0 in ((1, 255), (2, 256), (3, 299)):                              # the last slot observes what kf 0 lists at slot 255 / 256 / 299
        assert w["observes"][k][-1] == 1 and w["slots"][k][-1] == w["slots"][0][s0]
    assert w["slots"][0][10] in w["slots"][3] and np.flatnonzero(np.isin(w["slots"][3], w["slots"][0]) & (w["observes"][3] == 1)).max() == 129
    assert np.count_nonzero(np.isin(w["slots"][3][64:128], w["slots"][0])) > 0 and np.count_nonzero(np.isin(w["slots"][3][:64], w["slots"][0])) > 0
    assert cases.cov_weights(w, 0) == {1: 15, 2: 16, 3: 20} and by["cov_wide_keyframes"]["cov"][0] == dict(n_cov=2, n_connected=3, overflow=0, cov_kf=[2, 3], cov_weight=[16, 20])
    for K in (64, 65, 257):
        c, e = size[f"cov_K_{K}"], by[f"cov_K_{K}"]["cov"]
        assert len(c["worlds"][0]["slots"]) == K and [q[1] for q in c["cov"][:4]] == [0, 0, K - 1, K - 1]
        assert e[0]["cov_kf"] == [5, K - 57, K - 1, K // 2 + 1] and e[0]["cov_weight"] == [16, 17, 17, 18] and e[0]["n_connected"] == K - 1 and e[0]["overflow"] == 0
        assert e[1]["overflow"] == 1 and e[1]["cov_kf"] == e[0]["cov_kf"][:3] and e[2]["cov_kf"] == [3, 0, K - 2] and e[3]["overflow"] == 1 and e[3]["cov_kf"] == [3, 0]
    assert len(W("cov_K_65", 1)["slots"]) == 64 and [q[0] for q in size["cov_K_65"]["cov"][4:]] == [1, 1]
    e, wt = by["cov_K_257"]["cov"], cases.cov_weights(W("cov_K_257"), 1)
    assert 256 in e[0]["cov_kf"] and e[0]["cov_kf"].index(256) == 2                 # above the threshold, at its rank
    assert max(wt.values()) == 11 <= BR.COV_THRESHOLD and sorted(k for k in wt if wt[k] == 11) == [130, 256]      # the tie: 130 < 256 wins
    assert e[4] == dict(n_cov=1, n_connected=4, overflow=0, cov_kf=[130], cov_weight=[11]) and e[5]["overflow"] == 1 and e[5]["cov_kf"] == []
    c, w = size["cov_table_chains"], W("cov_table_chains")
    m = c["marks"]
    assert len(w["bad"]) == 24000
    table = cases.probe_table(cases.cov_listed(w, 0), cases.cov_home, 8192)
    H = m["H"]
    assert [cases.cov_home(p) for p in m["chain"]] == [H] * 4 and sorted(table[H + i] for i in range(4)) == sorted(m["chain"]) and H + 4 not in table
    assert cases.cov_home(m["miss"]) == H and m["miss"] not in w["slots"][0] and m["miss"] in w["slots"][1]
    assert cases.probe_find(table, cases.cov_home, 8192, m["miss"]) == (-1, [H, H + 1, H + 2, H + 3, H + 4])      # walks the chain, ends at an empty cell
    assert H <= cases.cov_home(m["bad"]) <= H + 3 and w["bad"][m["bad"]] == 1 and m["bad"] in w["slots"][0] and m["bad"] in w["slots"][1] and m["bad"] not in table.values()
    assert [cases.cov_home(p) for p in m["wrap"]] == [8191, 8191, 0] and {8191, 0, 1} <= set(table) and 2 not in table and 8190 not in table
    assert sorted(table[h] for h in (8191, 0, 1)) == sorted(m["wrap"]) and cases.probe_find(table, cases.cov_home, 8192, m["wrap"][2])[1][-1] >= 0
    assert max(len(cases.probe_find(table, cases.cov_home, 8192, p)[1]) for p in m["wrap"]) >= 2      # some point of the wrapping chain sits past its home cell
    assert cases.cov_home(m["miss_wrap"]) == 0 and cases.probe_find(table, cases.cov_home, 8192, m["miss_wrap"]) == (-1, [0, 1, 2]) and m["miss_wrap"] in w["slots"][2]
    assert cases.cov_weights(w, 0) == {1: 17, 2: 3} and by["cov_table_chains"]["cov"][0]["cov_kf"] == [1] and by["cov_table_chains"]["cov"][0]["cov_weight"] == [17]
    w = W("cov_table_full")
    listed = cases.cov_listed(w, 0)
    table = cases.probe_table(listed, cases.cov_home, 8192)
    assert len(listed) == len(set(listed)) == 4096 == len(table) and 2 * len(table) == 8192          # load 0.5
    assert max(len(cases.probe_find(table, cases.cov_home, 8192, p)[1]) for p in listed) >= 3         # and real chains in it
    assert set(w["slots"][1].tolist()) == set(listed) and not set(w["slots"][2].tolist()) & set(listed) and len(set(w["slots"][2].tolist())) == 4096
    assert cases.cov_weights(w, 0) == {1: 4096} and by["cov_table_full"]["cov"][0] == dict(n_cov=1, n_connected=1, overflow=0, cov_kf=[1], cov_weight=[4096])
    w = W("cov_table_full", 1)
    assert len(set(w["slots"][0].tolist())) == 1 and len(w["slots"][0]) == 4096 and int(w["observes"][1][w["slots"][1] == 7].sum()) == 1
    assert cases.cov_weights(w, 0) == {1: 4096} and by["cov_table_full"]["cov"][1]["cov_weight"] == [4096] and 4096 >= 1 << 12      # the 13th bit of the half word
    # -- window
    for E, bits in ((256, 9), (257, 10), (700, 11)):
        c, win = size[f"window_E_{E}"], by[f"window_E_{E}"]["windows"][0]
        w, (_, kf, cov, _, _, _, _) = c["worlds"][0], c["windows"][0]
        ent = cases.entries(w, kf, cov)
        good = [p for p in ent if p >= 0 and not w["bad"][p]]
        first = {e for e, p in enumerate(ent) if p >= 0 and not w["bad"][p] and p not in ent[:e]}
        assert len(cov) == 4 and len(ent) == E and cases.table_bits(E) == bits and win["usable"] == 1
        assert win["n_points"] == len(first) == len(set(good)) and win["n_obs"] > 256 and win["point_index"].tolist() == [ent[e] for e in sorted(first)]
        spec = cases.WINDOW_E[E]
        assert ent[spec["null_at"]] == -1 and w["bad"][ent[spec["bad_at"]]] == 1 and {spec["null_at"], spec["bad_at"]} & {255, 256}
        assert len(good) > len(first)                                               # points listed by several local keyframes
    assert 256 in {e for e, p in enumerate(cases.entries(W("window_E_257"), 6, [7, 8, 9, 10])) if p >= 0 and p not in cases.entries(W("window_E_257"), 6, [7, 8, 9, 10])[:e]}
    assert (cases.WINDOW_E[256]["bad_at"], cases.WINDOW_E[257]["null_at"], cases.WINDOW_E[700]["bad_at"], cases.WINDOW_E[700]["null_at"]) == (255, 255, 255, 256)
    ent, win = cases.entries(W("window_E_700"), 6, [7, 8, 9, 10]), by["window_E_700"]["windows"][0]
    first = [e for e, p in enumerate(ent) if p >= 0 and not W("window_E_700")["bad"][p] and p not in ent[:e]]
    assert all(any(lo <= e < lo + 256 for e in first) for lo in (0, 256, 512)) and win["n_points"] > 512 and win["n_points"] <= 800 and win["n_obs"] <= 3000
    assert ent[5] == ent[570] >= 0 and win["point_index"].tolist().count(ent[5]) == 1 and win["point_index"].tolist().index(ent[5]) == first.index(5)
    c, win = size["window_long_segments"], by["window_long_segments"]["windows"][0]
    w = c["worlds"][0]
    assert (win["n_local"], win["n_fixed"], win["usable"]) == (16, 60, 1) and c["windows"][0][3] == -1
    seg = np.bincount(win["obs_point"], minlength=win["n_points"])
    X = int(win["point_index"][120])
    assert seg.max() == seg[120] == 76 and sorted(int(s) >> 32 for s in win["obs_slot"][win["obs_point"] == 120]) == list(range(76))
    A, B = cases.LONG_A, cases.LONG_B
    in_window = lambda k: [(s, win["point_index"].tolist().index(int(p))) for s, (p, o) in enumerate(zip(w["slots"][k], w["observes"][k])) if o and p in win["point_index"]]
    assert len(w["slots"][A]) == 130 and in_window(A) == [(129, 120)] and w["slots"][A][129] == X
    assert in_window(B) == [(3, 101), (70, 11), (71, 120)]
    fixed = win["kf_index"][16:].tolist()
    keys = {k: min(i for _, i in in_window(k)) for k in fixed}
    assert fixed == sorted(fixed, key=lambda k: (keys[k], k)) and fixed[-1] == A and keys[B] == 11
    between = [k for k in fixed if 11 < keys[k] < 101]
    assert between and fixed.index(B) < fixed.index(between[0])                     # (with slot 70 lost, B would stand behind these)
    c, e = size["window_table_chains"], by["window_table_chains"]["windows"]
    m = c["marks"]
    for world, E, bits in ((0, 8, 4), (1, 9, 5)):
        ent = cases.entries(c["worlds"][world], 0, [1])
        assert len(ent) == E and cases.table_bits(E) == bits and ent.count(m["twice"]) == 2 and sorted(set(p for p in ent if p >= 0)) == sorted(m["chain"] + m["others"])
    home = lambda p: cases.win_home(p, 4)
    table = cases.probe_table([p for p in cases.entries(c["worlds"][0], 0, [1]) if p >= 0], home, 16)
    assert [home(p) for p in m["chain"]] == [14] * 5 and sorted(table[h] for h in (14, 15, 0, 1, 2)) == sorted(m["chain"]) and 3 not in table and 13 not in table
    assert home(m["miss"]) == 15 and cases.probe_find(table, home, 16, m["miss"]) == (-1, [15, 0, 1, 2, 3]) and m["miss"] in c["worlds"][0]["slots"][2]
    assert m["miss"] not in e[0]["point_index"] and e[0]["n_points"] == 7 and e[0]["n_fixed"] == 1
    other = cases.probe_table([p for p in cases.entries(c["worlds"][1], 0, [1]) if p >= 0], lambda p: cases.win_home(p, 5), 32)
    assert sorted(other) != sorted(table) and sorted(other.values()) == sorted(table.values())      # the same points in another table
    for k in cases.WINDOW_COLUMNS:
        assert np.asarray(e[0][k]).tobytes() == np.asarray(e[1][k]).tobytes(), k
    c, e = size["window_mixed_call"], by["window_mixed_call"]["windows"]
    assert [len(w["slots"]) for w in c["worlds"]] == [11, 6, 66] and len(cases.entries(c["worlds"][1], 4, [5])) == 5 and [x["usable"] for x in e] == [1, 1, 1]
    assert e[0]["n_points"] == by["window_E_700"]["windows"][0]["n_points"] and e[2]["n_fixed"] == 64 and c["windows"][2][1] == 64
    # -- commit
    for name, short in (("commit_many_points", 0), ("commit_many_points_bad_capacity_short_by_one", 1)):
        c, e = size[name], by[name]
        win, r, m = e["windows"][0], e["commits"][0], c["marks"]
        went = [win["point_index"].tolist().index(p) for p in BR.ba_commit(c["worlds"][0], win, win["T_c2w"], win["points"], e["flags"][0])[1]["bad_points"]]
        assert went == m["goes_bad"] and len(went) == r["n_bad"] > 256 and {255, 256} <= set(went) and all(any(lo <= i < lo + 256 for i in went) for lo in (0, 256, 512))
        assert r["overflow_bad"] == short and len(r["bad_points"]) == r["n_bad"] - short == c["bad_capacity"]
        hit = set(win["obs_point"][np.flatnonzero(e["flags"][0])].tolist())
        assert m["stays"] >= 512 and m["stays"] in hit and m["stays"] not in went and e["worlds_after"][0]["bad"][win["point_index"][m["stays"]]] == 0
        assert win["n_points"] <= 800 and win["n_obs"] <= 3000
    c, e = size["commit_overlap_beyond_256"], by["commit_overlap_beyond_256"]
    a, b = e["windows"]
    shared = set(a["point_index"].tolist()) & set(b["point_index"].tolist())
    assert a["usable"] and b["usable"] and shared == {c["marks"]["shared"]} and not set(a["kf_index"].tolist()) & set(b["kf_index"].tolist())
    assert a["point_index"].tolist().index(c["marks"]["shared"]) == 280 and b["point_index"].tolist().index(c["marks"]["shared"]) == 270
    assert e["overlap"] == (0, 1) == c["overlap"] and e["commits"] == [None, None]
    for w0, w1 in zip(c["worlds"], e["worlds_after"]):
        cases.same_world(w0, w1, "refused")


def test_the_chain_world_has_outliers_a_bad_point_and_a_good_point_with_an_outlier():
    """The world of the GPU chain test, solved by tests/local_ba_restatement.py: the property it was chosen for, confirmed on the CPU."""
    from tests import local_ba_restatement as R
    world, kf, cov, delta = cases.chain_world()
    win = BR.ba_window(world, kf, cov, -1)
    assert win["usable"] and win["n_fixed"] >= 1
    T, X, out, _ = R.solve(R.Problem(win["T_c2w"], win["kf_constant"], win["points"], win["obs_kf"], win["obs_point"], win["obs_bearing"], win["obs_level"], delta))
    _, r = BR.ba_commit(world, win, T.reshape(-1, 12), X, out)
    n_out, n_bad, good_with_outlier = cases.chain_property(win, out, r)
    assert n_out >= 1 and n_bad >= 1 and good_with_outlier >= 1, (n_out, n_bad, good_with_outlier)


def test_host_functions_agree_with_the_restatement(tmp_path):
    """update_connection_host, ba_window_host and ba_commit_host (plain C++, no device call) through the compiled driver on every case
    and on the chain world: integers equal, doubles bit-equal, and the map after the commits equal byte for byte. One job per world; its
    windows run in order on the map as the earlier commits left it (the overlapping case is committed by neither side)."""
    import struct
    jobs = []
    for c in EVERY:
        for m, world in enumerate(c["worlds"]):
            jobs.append((c["name"], world, [kf for w, kf, _ in c["cov"] if w == m],
                         [(spec, c["outliers"].get(i, []) if c["outliers"] is not None and not c["overlap"] else None) for i, spec in enumerate(c["windows"]) if spec[0] == m]))
    world, kf, cov, _ = cases.chain_world()
    jobs.append(("chain", world, [kf], [((0, kf, cov, -1, None, None, None), None)]))
    want = []
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(struct.pack("i", len(jobs)))
        for name, world, covs, windows in jobs:
            P, K = len(world["p_world"]), len(world["slots"])
            f.write(struct.pack("2i", P, K))
            f.write(np.ascontiguousarray(world["p_world"], np.float64).tobytes() + np.ascontiguousarray(world["bad"], np.uint8).tobytes())
            f.write(np.ascontiguousarray(world["found"], np.int32).tobytes() + np.ascontiguousarray(world["T_kf_w"], np.float64).tobytes())
            f.write(np.array([len(x) for x in world["slots"]], np.int32).tobytes())
            for key, dt in (("slots", np.int32), ("observes", np.uint8), ("px", np.float32), ("level", np.int32), ("bearing", np.float64)):
                for a in world[key]:
                    f.write(np.ascontiguousarray(a, dt).tobytes())
            f.write(struct.pack("i", len(covs)) + b"".join(struct.pack("i", k) for k in covs))
            f.write(struct.pack("i", len(windows)))
            now, wins = world, []
            for (_, k, cv, origin, kc, pc, oc), pairs in windows:
                win = BR.ba_window(now, k, cv, origin, kc, pc, oc)
                big = 1 << 30
                f.write(struct.pack("2i", k, len(cv)) + np.array(cv, np.int32).tobytes())
                commit = pairs is not None and win["usable"]
                f.write(struct.pack("5i", origin, big if kc is None else kc, big if pc is None else pc, big if oc is None else oc, int(commit)))
                r = None
                if commit:
                    flags = cases.flags_of(win, pairs)
                    f.write(flags.tobytes())
                    T, X = win["T_c2w"].copy(), win["points"] + 0.125
                    T[:, 3] += 0.25
                    now, r = BR.ba_commit(now, win, T, X, flags)
                wins.append((win, r))
            want.append((name, [BR.update_connection(world, k) for k in covs], wins, now))
    exe = str(tmp_path / "ba_window_driver")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "ba_window_host", "driver.cpp")], check=True)
    subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "answers.bin")], check=True)
    buf, at = open(tmp_path / "answers.bin", "rb").read(), 0

    def take(dt, n):
        nonlocal at
        a = np.frombuffer(buf, dt, n, at).copy()
        at += a.nbytes
        return a
    for name, covs, wins, after in want:
        for e in covs:
            n_connected, n = (int(v) for v in take(np.int32, 2))
            assert (n_connected, n) == (e["n_connected"], e["n_cov"]), name
            assert take(np.int32, n).tolist() == e["cov_kf"] and take(np.int32, n).tolist() == e["cov_weight"], name
        for win, r in wins:
            got = dict(zip(ba_window.RESULT_FIELDS, (int(v) for v in take(np.int32, 12))))
            if win["usable"]:
                nk, npt, no = win["n_local"] + win["n_fixed"], win["n_points"], win["n_obs"]
                got.update(kf_index=take(np.int32, nk), kf_constant=take(np.uint8, nk), T_c2w=take(np.float64, 12 * nk), point_index=take(np.int32, npt),
                           points=take(np.float64, 3 * npt), obs_kf=take(np.int32, no), obs_point=take(np.int32, no), obs_slot=take(np.int64, no),
                           obs_bearing=take(np.float64, 3 * no), obs_level=take(np.int32, no))
            cases.same_window(got, win, name)
            if r is not None:
                n_out, n_bad = (int(v) for v in take(np.int32, 2))
                assert (n_out, n_bad) == (r["n_outliers"], r["n_bad"]) and take(np.int32, n_bad).tolist() == r["bad_points"], name
        P, S = len(after["p_world"]), sum(len(x) for x in after["slots"])
        K = len(after["slots"])
        assert cases.same_bits(take(np.float64, 3 * P), np.asarray(after["p_world"], np.float64).reshape(-1)) and np.array_equal(take(np.uint8, P), after["bad"]), name
        assert cases.same_bits(take(np.float64, 12 * K), np.asarray(after["T_kf_w"], np.float64).reshape(-1)), name
        assert np.array_equal(take(np.int32, S), np.concatenate([np.asarray(x, np.int32) for x in after["slots"]] + [np.zeros(0, np.int32)])), name
        assert np.array_equal(take(np.uint8, S), np.concatenate([np.asarray(x, np.uint8) for x in after["observes"]] + [np.zeros(0, np.uint8)])), name
    assert at == len(buf)


def test_example_and_adapters_compile():
    """example_mapping.cpp uses KeyFrame::UpdateConnectionOnDevice and Optimizer::LocalBundleAdjustmentOnDevice of
    dsdtm_mapping_host.hpp and the host functions: the compiler sees them here."""
    path = os.path.join(ROOT, "dsdtm_amd", "host", "example_mapping.cpp")
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", path], check=True)
    src = open(path).read()
    assert "UpdateConnectionOnDevice(" in src and "LocalBundleAdjustmentOnDevice(" in src and "ba_window_host(" in src


def _lib_symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_declared_exported_and_mirrored(tmp_path):
    """The library exports exactly what its header declares and reads no environment; the ctypes mirror has the header's layouts and
    limits; the six older libraries export what their bindings list — libdsdtm_amd_trackmap.so its 11 symbols, from the one
    implementation now compiled twice."""
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_mapping.h")).read()
    for name, value in (("COV_THRESHOLD", BR.COV_THRESHOLD), ("MAX_PAIRS", BR.MAX_PAIRS), ("MAX_WINDOWS", BR.MAX_WINDOWS), ("MAX_COV", BR.MAX_COV)):
        assert re.search(r"#define DSDTM_MAPPING_%s %d\b" % (name, value), hdr) and getattr(ba_window, name) == value, name
    assert (BR.MAX_FREE_KF, BR.MAX_CONST_KF, BR.MAX_POINTS, BR.MAX_OBSERVATIONS) == (capi.LBA_MAX_FREE_KF, capi.LBA_MAX_CONST_KF, capi.LBA_MAX_POINTS, capi.LBA_MAX_OBSERVATIONS)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", code))
    assert declared == set(ba_window.SYMBOLS) and len(ba_window.SYMBOLS) == 14
    assert _lib_symbols(ba_window.lib_path()) == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", ba_window.lib_path()], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in und
    lib = ba_window.load()
    for sym in ba_window.SYMBOLS:
        decl = re.search(r"\b%s\(([^;]*?)\);" % sym, code, flags=re.S)
        assert decl and len(decl.group(1).split(",")) == len(getattr(lib, sym).argtypes), sym
    assert _lib_symbols(track_map.lib_path()) == set(track_map.SYMBOLS) and len(track_map.SYMBOLS) == 11
    assert _lib_symbols(local_map.lib_path()) == set(local_map.SYMBOLS) and _lib_symbols(capi.lib_path()) == set(capi.EXPORTED_SYMBOLS)
    assert _lib_symbols(motion.lib_path()) == set(motion.SYMBOLS) and _lib_symbols(homography.lib_path()) == set(homography.SYMBOLS)
    kf_hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsdtm_amd_keyframe.h")).read(), flags=re.S)
    assert _lib_symbols(os.path.join(ROOT, "dsdtm_amd", "csrc", "libdsdtm_amd_keyframe.so")) == set(re.findall(r"\b(dsdtm_[a-z0-9_]+)\s*\(", kf_hdr))
    structs = [("dsdtm_mapping_cov_desc", ba_window.CovDesc), ("dsdtm_mapping_cov_result", ba_window.CovResult), ("dsdtm_mapping_window_desc", ba_window.WindowDesc),
               ("dsdtm_mapping_window_arrays", ba_window.WindowArrays), ("dsdtm_mapping_window_result", ba_window.WindowResult),
               ("dsdtm_mapping_commit_result", ba_window.CommitResult), ("dsdtm_local_ba_problem", capi.LocalBaProblem)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "dsdtm_amd_mapping.h"', 'int main(void) {']
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
    hdr = open(os.path.join(ROOT, "include", "dsdtm_amd_mapping.h")).read()
    for needle in ("src/Keyframe.cpp:71-133", "src/Optimizer.cpp:109-159", "src/Optimizer.cpp:236-271", "src/MapPoint.cpp:57-109", "src/MapPoint.cpp:20",
                   "collects NO points", "THE FIRST\n *   TIME", "point_of_slot KEPT", "HAND ON THE USABLE WINDOWS ONLY", "lowest index wins", "counts twice",
                   "naming both windows", "pointer value"):
        assert needle in hdr, needle
