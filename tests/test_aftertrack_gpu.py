"""libdsdtm_amd_slam.so (include/dsdtm_amd_slam.h) on the MI355X: dsdtm_slam_track_commit against the restatement
(dsdtm_amd/aftertrack_restatement.py) on every case of tests/aftertrack_cases.py — counts, bad lists and found_after equal and the map,
read back before and after, equal to the restated one byte for byte — the order of descs, two maps in one call, a desc alone and as one
of eight, the commit in front of the next dsdtm_slam_local, every refusal, and the chain local -> track_frame -> commit against the
objects after tracking.apply_tracked_frame. No tolerance anywhere: every value is an integer or a copy."""
import ctypes as C

import numpy as np
import pytest

from dsdtm_amd import aftertrack_restatement as AR
from dsdtm_amd import slam, track_map, tracking
from dsdtm_amd import track_map_restatement as TR
from dsdtm_amd.frame import Config, Frame
from tests import aftertrack_cases as cases
from tests.ba_window_cases import same_world
from tests.local_map_cases import CAM

pytestmark = pytest.mark.gpu
INVALID = -2
FILL32 = int(np.full(4, slam.FILL, np.uint8).view(np.int32)[0])


@pytest.fixture(scope="module")
def sl_ctx():
    ctx = slam.SlamContext(0)
    yield ctx
    ctx.close()


def upload(ctx, world):
    m = ctx.new_map()
    m.points_write(0, world["p_world"], world["bad"], world["found"])
    for k in range(len(world["slots"])):
        assert m.keyframe_add(world["T_kf_w"][k], world["slots"][k], world["observes"][k], world["px"][k], world["level"][k], world["bearing"][k]) == k
    return m


def check_answers(call, got, want, name):
    cap = call.bad_capacity
    for t, (g, w) in enumerate(zip(got, want)):
        overflow = int(w["n_bad"] > cap)
        assert (g["n_erased"], g["n_bad"], g["overflow_bad"], g["reserved"]) == (w["n_erased"], w["n_bad"], overflow, 0), (name, t, g, w)
        assert g["bad_points"] == w["bad_points"][:cap] and g["found_after"] == w["found_after"], (name, t, g, w)
        row, fa = g["raw"]
        assert np.all(row[min(w["n_bad"], cap):] == FILL32) and np.all(fa[len(w["found_after"]):] == FILL32), (name, t)      # behind what the result reports: untouched


def run_case(ctx, c, descs=None):
    """Upload the case's worlds, read them back, commit, read back again; everything against the restatement."""
    descs = c["descs"] if descs is None else descs
    after, want = AR.track_commit_call(c["worlds"], c["threshold"], descs)
    maps = [upload(ctx, w) for w in c["worlds"]]
    try:
        for m, w in zip(maps, c["worlds"]):
            same_world(m.read(), w, (c["name"], "before"))
        call = slam.CommitCall(ctx, c["threshold"], [(maps[m], p, r) for m, p, r in descs], c["bad_capacity"])
        ctx.check(call.run_raw())
        got = call.answers()
        check_answers(call, got, want, c["name"])
        reads = [m.read() for m in maps]
        for r, w in zip(reads, after):
            same_world(r, w, (c["name"], "after"))
        return got, reads
    finally:
        for m in maps:
            m.close()


@pytest.mark.parametrize("c", cases.all_cases(), ids=lambda c: c["name"])
def test_every_case_equals_the_restatement(sl_ctx, c):
    run_case(sl_ctx, c)


def test_what_the_named_cases_do_on_the_device(sl_ctx):
    """The edges by their own numbers, read from the device's answers (the restated ones are asserted by the CPU half)."""
    got, reads = run_case(sl_ctx, cases.by_name("equal_is_kept_next_double_is_erased_nan_is_kept"))
    assert got[0]["found_after"] == [4, 3, 4, 3] and got[0]["n_bad"] == 0
    c = cases.by_name("found_zero_goes_bad_three_observers_cleared_the_listed_slot_kept")
    got, reads = run_case(sl_ctx, c)
    p = c["marks"]["point"]
    assert got[0]["bad_points"] == [p] and reads[0]["bad"][p] == 1 and reads[0]["found"][p] == 0
    assert [int(np.count_nonzero(s == p)) for s in reads[0]["slots"]] == [0, 0, 0, 1, 0]
    c = cases.by_name("a_point_bad_before_the_call_is_incremented_only")
    got, reads = run_case(sl_ctx, c)
    assert got[0]["found_after"][0] == 1 and got[0]["n_bad"] == 0 and sum(int(np.count_nonzero((s == 1) & (o == 1))) for s, o in zip(reads[0]["slots"], reads[0]["observes"])) == 4
    got, _ = run_case(sl_ctx, cases.by_name("256_matches_bad_capacity_short_by_one"))
    assert got[0]["overflow_bad"] == 1 and len(got[0]["bad_points"]) == got[0]["n_bad"] - 1
    c = cases.by_name("slot_pool_over_several_blocks")
    got, reads = run_case(sl_ctx, c)
    flat = cases.flat(reads[0], "slots", np.int32)
    assert got[0]["n_bad"] == 3 and flat[[0, 255, 256, 300, 917, 1799]].tolist() == [-1] * 6 and np.count_nonzero(flat >= 0) == 18


def test_desc_order_decides_and_swapped_descs_differ_as_restated(sl_ctx):
    a, b = cases.by_name("two_descs_share_a_point_in_order"), cases.by_name("two_descs_share_a_point_swapped")
    (ga, ra), (gb, rb) = run_case(sl_ctx, a), run_case(sl_ctx, b)
    assert ga[0]["bad_points"] == [0] and ga[1]["found_after"] == [3, 1, 1] and ga[1]["n_bad"] == 0        # desc 1 increments the bad point only
    assert gb[0]["bad_points"] == [0, 6] and gb[0]["found_after"] == [2, 0, 0] and gb[1]["n_erased"] == 0
    assert ra[0]["bad"][6] == 0 and rb[0]["bad"][6] == 1


def test_a_desc_alone_and_as_one_of_eight_gives_the_same_bytes(sl_ctx):
    """Two maps in one call; the first desc of each map alone equals that desc in the call of eight (it meets the untouched map both
    times), and the two maps alone, each with its own descs, end as they end in the joint call."""
    c = cases.by_name("two_maps_eight_descs")
    got8, reads8 = run_case(sl_ctx, c)
    for first in (0, 1):
        got1, _ = run_case(sl_ctx, c, [c["descs"][first]])
        for k in ("n_erased", "n_bad", "bad_points", "found_after"):
            assert got1[0][k] == got8[first][k], (first, k)
    for m in (0, 1):
        mine = [d for d in c["descs"] if d[0] == m]
        got, reads = run_case(sl_ctx, c, mine)
        same_world(reads[m], reads8[m], ("map alone", m))
        assert [g["found_after"] for g in got] == [g["found_after"] for g, d in zip(got8, c["descs"]) if d[0] == m]


def test_no_desc_and_a_lost_frame(sl_ctx):
    w = cases.by_name("a_lost_frame_has_no_matches")["worlds"][0]
    m = upload(sl_ctx, w)
    try:
        assert sl_ctx.lib.dsdtm_slam_track_commit(sl_ctx.handle, cases.THR, 0, None, 0, None, None) == 0
        res = (slam.CommitResult * 1)()
        d = (slam.CommitDesc * 1)()
        d[0].map, d[0].n_matches = m.handle, 0
        assert sl_ctx.lib.dsdtm_slam_track_commit(sl_ctx.handle, cases.THR, 1, d, 0, None, res) == 0
        assert (res[0].n_erased, res[0].n_bad, res[0].overflow_bad, res[0].reserved) == (0, 0, 0, 0)
        same_world(m.read(), w, "lost frame")
    finally:
        m.close()


def test_the_commit_is_in_front_of_the_next_local(sl_ctx):
    """commit, then dsdtm_slam_local with nothing in between (no read, no wait of the caller's): the columns carry the new found counts and
    the point that went bad is gone — what the restated local answers on the restated world."""
    c = cases.by_name("found_zero_goes_bad_three_observers_cleared_the_listed_slot_kept")
    w, p = c["worlds"][0], c["marks"]["point"]
    T = np.asarray(w["T_kf_w"][0], np.float64)
    (after,), _ = cases.expected(c)
    m = upload(sl_ctx, w)
    try:
        before = sl_ctx.local(CAM, [(m, T, 64, 256)])[0]
        assert p in before["point"]
        call = slam.CommitCall(sl_ctx, c["threshold"], [(m, d[1], d[2]) for d in c["descs"]])
        local = track_map.LocalCall(sl_ctx, CAM, [(m, T, 64, 256)])
        assert call.run_raw() == 0 and local.run_raw() == 0
        got = local.answers()[0]
        want = TR.track_map_local(CAM, T, after, 10, 0, 64, 256)
        assert got["point"] == want["point"] and p not in got["point"] and 0 in got["point"]
        assert got["flat"]["found"].tolist() == [int(after["found"][q]) for q in got["point"]]
        assert got["flat"]["found"][got["point"].index(0)] == w["found"][0] + 1
    finally:
        m.close()


def test_refused_calls_leave_map_and_outputs_untouched(sl_ctx):
    w = cases.base().world()
    other = slam.SlamContext(0)
    m, foreign = upload(sl_ctx, w), other.new_map()
    try:
        P = len(w["bad"])
        good = (m, [0, 1, 2], [1.0, 1.0, 1.0])
        refusals = [(cases.THR, [good, (foreign, [], [])], None, "desc 1: map is not a map of this context"),
                    (cases.THR, [good, (m, [0, P], [1.0, 1.0])], None, "desc 1: point[1]"), (cases.THR, [good, (m, [-1], [1.0])], None, "desc 1: point[0] = -1"),
                    (cases.THR, [good, (m, [3, 4, 3], [1.0, 1.0, 1.0])], None, "desc 1: point 3 occurs twice"),
                    (cases.THR, [good, (m, [i % P for i in range(257)], [0.0] * 257)], None, "desc 1: n_matches"),
                    (float("nan"), [good], None, "not finite"), (float("inf"), [good], None, "not finite"), (cases.THR, [good], -1, "bad_capacity"),
                    (cases.THR, [good] * 1025, None, "outside")]
        for thr, frames, cap, needle in refusals:
            call = slam.CommitCall(sl_ctx, thr, frames, cap)
            assert call.run_raw() == INVALID and needle in sl_ctx.last_error(), (needle, sl_ctx.last_error())
            assert np.all(call.bad.view(np.uint8) == slam.FILL) and bytes(call.results) == bytes([slam.FILL]) * C.sizeof(call.results), needle
            assert all(np.all(fa.view(np.uint8) == slam.FILL) for _, _, fa in call.keep), needle
            same_world(m.read(), w, needle)
        call = slam.CommitCall(sl_ctx, cases.THR, [good])
        lib, h = sl_ctx.lib, sl_ctx.handle
        for args, needle in (((h, cases.THR, 1, None, 3, call.bad.ctypes.data, call.results), "descs is NULL"), ((h, cases.THR, 1, call.descs, 3, None, call.results), "bad_points is NULL"),
                             ((h, cases.THR, 1, call.descs, 3, call.bad.ctypes.data, None), "results is NULL")):
            assert lib.dsdtm_slam_track_commit(*args) == INVALID and needle in sl_ctx.last_error(), needle
        assert lib.dsdtm_slam_track_commit(None, cases.THR, 1, call.descs, 3, call.bad.ctypes.data, call.results) == INVALID
        for field, needle in (("map", "map is NULL"), ("point", "point is NULL"), ("residual_norm", "residual_norm is NULL")):
            call = slam.CommitCall(sl_ctx, cases.THR, [good])
            setattr(call.descs[0], field, None)
            assert call.run_raw() == INVALID and needle in sl_ctx.last_error(), needle
        same_world(m.read(), w, "NULL arguments")
    finally:
        m.close()
        foreign.close()
        other.close()


def test_the_mapping_entries_serve_the_same_map(sl_ctx):
    """The map the commit wrote is the map dsdtm_slam_covisibility reads: a point that went bad no longer counts (rule weights of
    include/dsdtm_amd_mapping.h), as restated on the restated world."""
    from dsdtm_amd import ba_window_restatement as BR
    c = cases.by_name("two_descs_share_a_point_swapped")
    (after,), _ = cases.expected(c)
    m = upload(sl_ctx, c["worlds"][0])
    try:
        before = sl_ctx.covisibility([(m, 0, 8)])[0]
        sl_ctx.track_commit(c["threshold"], [(m, d[1], d[2]) for d in c["descs"]])
        got, want = sl_ctx.covisibility([(m, 0, 8)])[0], BR.update_connection(after, 0)
        assert (got["cov_kf"], got["cov_weight"], got["n_connected"]) == (want["cov_kf"], want["cov_weight"], want["n_connected"]) and got["cov_weight"] != before["cov_weight"]
    finally:
        m.close()


def test_chain_local_track_frame_commit_equals_the_objects(gpu_ctx, sl_ctx):
    """TrackMapStore over a SlamContext -> dsdtm_slam_local -> dsdtm_track_frame -> tracking.apply_tracked_frame on the objects and
    Tracker.CommitTrackedFrame on the device, on the small synthetic search world of the track-map tests: the map read back equals the
    map rebuilt from the objects (store.mirror()). The keyframe side of SetBadFlag, which apply_tracked_frame leaves to the map's
    owner, is done on the objects here from the source (src/MapPoint.cpp:98-105). The threshold is set to the median norm, and every
    fourth local point starts with a found count of 0, so that erases and bad points happen."""
    from tests.test_search_gpu import make_world
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    cam, kfs, cur, mps = make_world(21, n_points=700, n_kf=2)
    for k, kf in enumerate(kfs):
        mpts = [None] * kf.n_features
        for mp in mps:
            if k in mp.mObservations:
                mpts[mp.mObservations[k]] = mp
        kf.mvMapPoints = mpts
    for i, mp in enumerate(mps):
        if i % 4 == 0:
            mp.mnFound = 0
    store = track_map.TrackMapStore(sl_ctx)
    for kf in kfs:
        store.add_keyframe(kf)
    T = cur.Get_Pose()
    r = store.local(cam, T)
    last = Frame(cam, cur.mvImg_Pyr, T)
    t = tracking.Tracker(cam, gpu_ctx, 5, 0, 8)
    res = tracking.track_frame(gpu_ctx, cam, cur.mvImg_Pyr[0], 5, last, T, (5, 0, 8, 15), 0, store.keyframes, r["map_points"], flat=r["flat"])
    keep = Config.Get("Optimization.LocalBAthreshhold")
    try:
        assert not res["lost"] and len(res["matches"]) > 20
        Config.Set("Optimization.LocalBAthreshhold", float(np.median(res["residual_norm"])) * float(cam.f))
        matched = [r["map_points"][int(i)] for i in res["matches"]["point"]]
        observers = {id(mp): dict(mp.mObservations) for mp in matched}
        was_bad = {id(mp): mp.IsBad() for mp in matched}
        tracking.apply_tracked_frame(cam, cur.mvImg_Pyr[0], res, r["map_points"])
        went_bad = [mp for mp in matched if mp.IsBad() and not was_bad[id(mp)]]
        for mp in went_bad:
            for k, s in observers[id(mp)].items():
                kfs[k].mvMapPoints[s] = None
        ans = t.CommitTrackedFrame(store, res, r["point"])
        assert ans["n_erased"] > 5 and ans["n_bad"] == len(went_bad) > 0 and ans["bad_points"] == [store.point_index(mp) for mp in went_bad]
        assert ans["found_after"] == [mp.Get_FoundNums() for mp in matched]
        same_world(store.map.read(), store.mirror(), "chain")
    finally:
        Config.Set("Optimization.LocalBAthreshhold", keep)
        res["frame"].close()


# ---- dsdtm_slam_need_keyframes ------------------------------------------------------------------------------------------------------
def keyframe_trackers(maps, kcs):
    return [dict(t, map=m) for m, (_, _, t) in zip(maps, kcs)]


@pytest.fixture(scope="module")
def keyframe_answers(gpu_ctx, sl_ctx):
    """Every keyframe case once: the entry on the resident map (each tracker alone: its own params), dsdtm_need_keyframes on the
    host-gathered arrays, keyframe_decision on the same arrays. Shared by the tests below and never changed."""
    from dsdtm_amd import capi
    from tests import need_keyframe_cases as NK
    out = {}
    for name, world, t in cases.keyframe_cases():
        m = upload(sl_ctx, world)
        try:
            call = slam.KeyframeCall(sl_ctx, t["cam"], t["params"], [dict(t, map=m)])
            assert call.run_raw() == 0, sl_ctx.last_error()
            g = cases.gathered(world, t)
            host = capi.KeyframeCall(gpu_ctx, t["cam"], t["params"], [NK.desc_of(g)])
            assert host.run_raw() == 0
            out[name] = dict(device=call.answers()[0], device_bytes=call.verdicts[:1].tobytes(), host=host.run()[0], host_bytes=host.verdicts[:1].tobytes(),
                             reference=NK.run_reference(g))
        finally:
            m.close()
    return out


@pytest.mark.parametrize("name", [k[0] for k in cases.keyframe_cases()])
def test_verdict_bytes_equal_need_keyframes_on_the_host_gathered_arrays(keyframe_answers, name):
    a = keyframe_answers[name]
    assert a["device_bytes"] == a["host_bytes"], (name, a["device"], a["host"])


@pytest.mark.parametrize("name", [k[0] for k in cases.keyframe_cases()])
def test_decisions_equal_keyframe_decision(keyframe_answers, name):
    """Integers equal, the two medians bit-equal, the other quantities within the 1e-9 the existing entry is held to."""
    from tests import need_keyframe_cases as NK
    got, want = keyframe_answers[name]["device"], keyframe_answers[name]["reference"]
    if want["undefined"]:               # (include/dsdtm_amd_keyframe.h: the other fields of such a verdict are unspecified)
        assert got["undefined"] == 1, (name, got)
        return
    NK.assert_same_verdict(got, want, name, rtol=1e-9)


def test_the_keyframe_cases_decide_what_they_are_named_for(keyframe_answers):
    a = keyframe_answers
    assert [a[k]["device"]["reason"] for k in ("k1_decides", "k2_decides", "k3_decides", "k4_decides", "k4_fabs_quirk")] == [1, 2, 3, 4, 0]
    assert a["forty_slots_holes_and_bad_31_sample_cut"]["device"]["n_px"] == 31 and a["empty_lists"]["device"]["n_px"] == 0 and a["empty_lists"]["device"]["n_depth"] == 0
    assert a["64_local_keyframes_last_fires"]["device"]["svo_kf"] == 63 and a["no_local_keyframe"]["device"]["svo_kf"] == -1
    assert a["a_point_at_z_0_is_undefined"]["device"]["undefined"] == 1 and a["all_bad"]["device"]["n_depth"] == 0
    assert 0 < a["bad_points_in_the_cur_list"]["device"]["n_depth"] < 40 and 3000 < a["4096_cur_points"]["device"]["n_depth"] < 4096


def test_trackers_of_several_maps_in_one_call_equal_each_alone(sl_ctx, keyframe_answers):
    """Every case with the default parameters in ONE call, one map per tracker and two trackers on the first map: each verdict has the
    bytes it has alone."""
    from dsdtm_amd.keyframe_decision import KeyframeParams
    kcs = [k for k in cases.keyframe_cases() if k[2]["params"] == KeyframeParams()]
    assert len(kcs) >= 6
    maps = [upload(sl_ctx, w) for _, w, _ in kcs]
    try:
        trackers = keyframe_trackers(maps, kcs) + [dict(kcs[0][2], map=maps[0])]
        call = slam.KeyframeCall(sl_ctx, kcs[0][2]["cam"], KeyframeParams(), trackers)
        assert call.run_raw() == 0, sl_ctx.last_error()
        for i, (name, _, _) in enumerate(kcs + [kcs[0]]):
            assert call.verdicts[i:i + 1].tobytes() == keyframe_answers[name]["device_bytes"], name
    finally:
        for m in maps:
            m.close()


def test_a_commit_changes_the_next_keyframe_decision(sl_ctx):
    """The two entries on one map: a point of the last keyframe that goes bad through the commit (T3 nulls its slot) is out of the
    next decision's list, as restated on the restated world."""
    from tests import need_keyframe_cases as NK
    name, world, t = [k for k in cases.keyframe_cases() if k[0] == "small_then_huge_20"][0]
    world = dict(world, found=np.zeros(len(world["bad"]), np.int32))
    (after,), r = AR.track_commit_call([world], cases.THR, [(0, [0, 1, 2, 3, 4, 25], [cases.HIGH] * 5 + [cases.LOW])])
    m = upload(sl_ctx, world)
    try:
        before = sl_ctx.need_keyframes(t["cam"], t["params"], [dict(t, map=m)])[0]
        got = sl_ctx.track_commit(cases.THR, [(m, [0, 1, 2, 3, 4, 25], [cases.HIGH] * 5 + [cases.LOW])])[0]
        assert got["bad_points"] == r[0]["bad_points"] == [0, 1, 2, 3, 4]
        now = sl_ctx.need_keyframes(t["cam"], t["params"], [dict(t, map=m)])[0]
        NK.assert_same_verdict(now, NK.run_reference(cases.gathered(after, t)), "after the commit")
        assert before["median_px"] == 8.0 and now["median_px"] == 4096.0           # of the first 31 good ones 20 are small, then 15: the element at index 15 moves
    finally:
        m.close()


def test_refused_keyframe_calls_leave_the_verdicts_untouched(sl_ctx):
    name, world, t = cases.keyframe_cases()[3]
    other = slam.SlamContext(0)
    m, foreign = upload(sl_ctx, world), other.new_map()
    try:
        P, K = len(world["bad"]), len(world["slots"])
        good = dict(t, map=m)
        refusals = [(dict(good, map=foreign), "tracker 1: map is not a map of this context"), (dict(good, kf=K), "tracker 1: kf is not"), (dict(good, kf=-1), "tracker 1: kf is not"),
                    (dict(good, cur_point=[0, P]), "tracker 1: cur_point[1]"), (dict(good, cur_point=[-1]), "tracker 1: cur_point[0] = -1"),
                    (dict(good, local_kf=[K]), "tracker 1: local_kf[0]"), (dict(good, T_cur_w=np.full(12, np.inf)), "tracker 1: T_cur_w is not finite"),
                    (dict(good, cur_point=[0] * 4097), "tracker 1: n_cur_points"), (dict(good, local_kf=[0] * 65), "tracker 1: n_local_kf")]
        for bad, needle in refusals:
            call = slam.KeyframeCall(sl_ctx, t["cam"], t["params"], [good, bad])
            assert call.run_raw() == INVALID and needle in sl_ctx.last_error(), (needle, sl_ctx.last_error())
            assert np.all(call.verdicts.view(np.uint8) == slam.FILL), needle
        call = slam.KeyframeCall(sl_ctx, t["cam"], t["params"], [good] * 1025)
        assert call.run_raw() == INVALID and "outside" in sl_ctx.last_error() and np.all(call.verdicts.view(np.uint8) == slam.FILL)
        call = slam.KeyframeCall(sl_ctx, t["cam"], t["params"], [good])
        call.prm.px_samples = 65
        assert call.run_raw() == INVALID and "px_samples" in sl_ctx.last_error() and np.all(call.verdicts.view(np.uint8) == slam.FILL)
        for field, needle in (("map", "map is NULL"), ("T_cur_w", "T_cur_w is NULL"), ("cur_point", "cur_point is NULL"), ("local_kf", "local_kf is NULL")):
            call = slam.KeyframeCall(sl_ctx, t["cam"], t["params"], [good])
            setattr(call.descs[0], field, None)
            assert call.run_raw() == INVALID and needle in sl_ctx.last_error(), needle
        lib, h = sl_ctx.lib, sl_ctx.handle
        assert lib.dsdtm_slam_need_keyframes(h, None, C.byref(call.prm), 1, call.descs, call.verdicts.ctypes.data) == INVALID and "cam is NULL" in sl_ctx.last_error()
        assert lib.dsdtm_slam_need_keyframes(h, C.byref(call.cam), C.byref(call.prm), 1, call.descs, None) == INVALID and "verdicts is NULL" in sl_ctx.last_error()
        assert lib.dsdtm_slam_need_keyframes(h, C.byref(call.cam), C.byref(call.prm), 0, None, None) == 0
        same_world(m.read(), world, "refused keyframe calls")
    finally:
        m.close()
        foreign.close()
        other.close()


def test_multitracker_need_keyframes_on_map_equals_need_keyframes(gpu_ctx, sl_ctx):
    """MultiTracker.NeedKeyframesOnMap on a TrackMapStore against MultiTracker.NeedKeyframes on the same objects: integers equal, the
    medians bit-equal, the rest within 1e-9 (the camera centres are the same formula in another association)."""
    from types import SimpleNamespace
    from tests import need_keyframe_cases as NK
    from tests.ba_window_cases import World
    b = World(61)
    k = [b.kf(24) for _ in range(4)]
    for kf in k:
        for _ in range(12):
            b.point(kf)
    b.share(k[3], k[1], 6)
    b.mps[40].SetBadFlag()
    store = track_map.TrackMapStore(sl_ctx)
    for kf in k:
        store.add_keyframe(kf)
    T = np.array(k[3].Get_Pose(), np.float64).reshape(3, 4)
    T[0, 3] += 0.3
    cur = SimpleNamespace(Get_Pose=lambda: T, mvMapPoints=[mp for mp in k[3].mvMapPoints[:10]] + [None, b.mps[40]])
    mt = tracking.MultiTracker(NK.CAM, gpu_ctx, 5, 0, 8)
    prm = mt.t.keyframe_params()
    got = mt.NeedKeyframesOnMap([store, store], [cur, cur], [k[3], k[1]], [[k[0], k[2]], []], prm)
    want = mt.NeedKeyframes([cur, cur], [k[3], k[1]], [[k[0], k[2]], []], prm)
    for g, w in zip(got, want):
        NK.assert_same_verdict(g, w, "on the map against the objects")
    assert got[0]["n_px"] == 17 and got[0]["n_depth"] == 9 and got[1]["svo_kf"] == -1           # 18 listed, one of them bad; 11 cur points, the bad one twice
