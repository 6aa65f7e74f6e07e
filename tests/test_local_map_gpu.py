"""dsdtm_localmap_select and the device-resident map (include/dsdtm_amd_localmap.h) on the MI355X against the restatement
(dsdtm_amd/local_map_restatement.py) on the cases of tests/local_map_cases.py: kf, point, point_kf and the four counters equal,
kf_dist bit-equal — no tolerance, every operation involved (+ - x / sqrt in double without contraction, a float narrowing, rint) is
correctly rounded on both sides. Then the batch, the update path with its re-allocations, map_read, the argument checks and the
Python path into dsdtm_track_frame."""
import copy

import numpy as np
import pytest

from dsdtm_amd import local_map, tracking
from dsdtm_amd import local_map_restatement as R
from dsdtm_amd.frame import Config, Frame
from tests import local_map_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm_ctx():
    ctx = local_map.LocalMapContext(0)
    yield ctx
    ctx.close()


def upload(ctx, world, piece=None):
    m = ctx.new_map()
    P = len(world["p_world"])
    piece = piece or max(P, 1)
    for a in range(0, P, piece):
        m.points_write(a, world["p_world"][a:a + piece], world["bad"][a:a + piece])
    for k, s in enumerate(world["slots"]):
        assert m.keyframe_add(world["T_kf_w"][k], s) == k
    return m


def check_guards(got, want, cap, n_local):
    """Nothing is written past what the call reports: the rest of every output array still holds the fill bytes."""
    fill32, raw = np.full(1, local_map.FILL, np.uint8).repeat(4).view(np.int32)[0], got["raw"]
    m = min(want["n_points"], cap)
    assert (raw["point"][m:] == fill32).all() and (raw["point_kf"][m:] == fill32).all() and (raw["kf"][want["n_kf"]:] == fill32).all()
    assert (raw["kf_dist"][want["n_kf"]:].view(np.uint8) == local_map.FILL).all()
    assert len(raw["kf"]) == n_local


@pytest.mark.parametrize("c", cases.all_cases(), ids=lambda c: c["name"])
def test_select_equals_the_restatement(lm_ctx, c):
    m = upload(lm_ctx, c["world"])
    wants = cases.expected(c)
    for q, (T, want) in enumerate(zip(c["poses"], wants)):
        cap = cases.capacity_of(c, want)
        got = lm_ctx.select(cases.CAM, [(m, T, cap)], c["n_local"], c["boundary"])[0]
        cases.same_answer(got, want, (c["name"], q))
        check_guards(got, want, cap, c["n_local"])
    # all poses of the case in one call: each result equal to its single call
    caps = [cases.capacity_of(c, w) for w in wants]
    for q, got in enumerate(lm_ctx.select(cases.CAM, [(m, T, cap) for T, cap in zip(c["poses"], caps)], c["n_local"], c["boundary"])):
        cases.same_answer(got, wants[q], (c["name"], "batch", q))
    m.close()


def test_map_read_returns_what_was_written(lm_ctx):
    c = [c for c in cases.all_cases() if c["name"] == "duplicates_within_a_keyframe"][0]
    w = c["world"]
    m = upload(lm_ctx, w, piece=150)
    got = m.read()
    assert np.array_equal(got["p_world"].view(np.uint64), np.ascontiguousarray(w["p_world"]).view(np.uint64)) and np.array_equal(got["bad"], w["bad"])
    assert np.array_equal(got["T_kf_w"], w["T_kf_w"]) and len(got["slots"]) == len(w["slots"])
    assert all(np.array_equal(a, b) for a, b in zip(got["slots"], w["slots"]))
    empty = lm_ctx.new_map()
    assert [len(v) for v in empty.read().values()] == [0, 0, 0, 0]
    empty.close()
    m.close()


def test_batch_of_different_maps_equals_the_single_calls(lm_ctx):
    by = {c["name"]: c for c in cases.all_cases()}
    a, b, e = by["duplicates_within_a_keyframe"], by["n_local_64_of_70"], by["empty_map"]
    ma, mb, me = (upload(lm_ctx, c["world"]) for c in (a, b, e))
    T2 = cases.pose((0.25, 0.0, -0.5), yaw=0.05)
    queries = [(ma, cases.I12, 500, a), (me, cases.I12, 4, e), (mb, cases.I12, 300, b), (ma, T2, 500, a), (mb, cases.I12, 3, b), (mb, T2, 7, b)]
    got = lm_ctx.select(cases.CAM, [(m, T, cap) for m, T, cap, _ in queries], 5, 0)
    for i, (m, T, cap, c) in enumerate(queries):
        want = R.select_local_map(cases.CAM, T, c["world"], 5, 0, cap)
        cases.same_answer(got[i], want, i)
        check_guards(got[i], want, cap, 5)
        cases.same_answer(lm_ctx.select(cases.CAM, [(m, T, cap)], 5, 0)[0], want, ("single", i))
    assert got[4]["overflow"] == 1 and got[0]["kf_dist"] != got[3]["kf_dist"]
    for m in (ma, mb, me):
        m.close()


def test_incremental_life_of_a_map(lm_ctx):
    """Points appended in pieces, keyframes added, a pose rewritten, slots rewritten to -1 and to new points, bad flags set, growth
    across the initial capacity of points, keyframes and slots: after every step the device selection equals the restatement on
    the host's mirror, and at the end map_read returns the mirror."""
    rng = np.random.default_rng(11)
    m = lm_ctx.new_map()
    w = dict(p_world=np.zeros((0, 3)), bad=np.zeros(0, np.uint8), T_kf_w=np.zeros((0, 12)), slots=[])
    poses = [cases.I12, cases.pose((0.5, 0, 0.25), yaw=0.4)]

    def check(step):
        for T in poses:
            want = R.select_local_map(cases.CAM, T, w, 6, 0)
            cap = max(1, want["n_points"])
            cases.same_answer(lm_ctx.select(cases.CAM, [(m, T, cap)], 6, 0)[0], want, step)

    def add_points(n):
        X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1, 1, n), rng.uniform(-1.0, 4.0, n)], 1)
        m.points_write(len(w["p_world"]), X, np.zeros(n, np.uint8))
        w["p_world"], w["bad"] = np.vstack([w["p_world"], X]), np.concatenate([w["bad"], np.zeros(n, np.uint8)])

    def add_kf(ns):
        s = rng.integers(-1, len(w["p_world"]), ns).astype(np.int32)
        T = np.array(cases.pose(tuple(rng.integers(-4, 5, 3) * 0.5)))
        assert m.keyframe_add(T, s) == len(w["slots"])
        w["T_kf_w"] = np.vstack([w["T_kf_w"], T[None]])
        w["slots"].append(s)
    check("empty")
    for n in (1, 63, 300):                                   # 1. points in pieces
        add_points(n)
    check("points only")
    for ns in (0, 1, 40, 300):                               # 2. keyframes
        add_kf(ns)
        check(f"keyframe of {ns} slots")
    w["T_kf_w"][2] = cases.pose((0.125, 0, 0))               # 3. a pose rewritten
    m.keyframe_write(2, w["T_kf_w"][2])
    check("pose rewritten")
    w["slots"][3][10:50] = -1                                # 4. slots rewritten: to -1, to new points, pose and slots together
    m.keyframe_write(3, None, 10, w["slots"][3][10:50])
    add_points(20)
    w["slots"][3][100:120] = np.arange(len(w["p_world"]) - 20, len(w["p_world"]))
    w["T_kf_w"][3] = cases.pose((0.125, 0, 0))
    m.keyframe_write(3, w["T_kf_w"][3], 100, w["slots"][3][100:120])
    check("slots rewritten")
    flagged = rng.choice(len(w["p_world"]), 60, replace=False)          # 5. bad flags, one point at a time and as a run
    for p in flagged[:5]:
        w["bad"][p] = 1
        m.points_write(int(p), w["p_world"][p:p + 1], w["bad"][p:p + 1])
    w["bad"][100:160] = 1
    w["p_world"][100:160] += 0.01
    m.points_write(100, w["p_world"][100:160], w["bad"][100:160])
    check("bad flags")
    assert len(w["p_world"]) < local_map.INITIAL_POINTS and len(w["slots"]) < local_map.INITIAL_KEYFRAMES      # 6. growth
    add_points(local_map.INITIAL_POINTS - len(w["p_world"]) - 1)
    add_points(2)                                            # across the point capacity with one small write
    check("points grown")
    add_points(local_map.INITIAL_POINTS + 5)                 # more than double at once
    while len(w["slots"]) <= local_map.INITIAL_KEYFRAMES:    # across the keyframe capacity; the slot pool grows on the way
        add_kf(300)
    assert sum(len(s) for s in w["slots"]) > local_map.INITIAL_SLOTS
    check("keyframes and slots grown")
    got = m.read()
    assert np.array_equal(got["p_world"], w["p_world"]) and np.array_equal(got["bad"], w["bad"]) and np.array_equal(got["T_kf_w"], w["T_kf_w"])
    assert all(np.array_equal(a, b) for a, b in zip(got["slots"], w["slots"]))
    m.close()


def test_refused_calls_leave_map_and_outputs_untouched(lm_ctx):
    c = [c for c in cases.all_cases() if c["name"] == "point_in_two_chosen_keyframes"][0]
    m, other = upload(lm_ctx, c["world"]), local_map.LocalMapContext(0)
    foreign = other.new_map()
    before = m.read()

    def refused(fn, *needles):
        with pytest.raises(local_map.LocalMapError) as e:
            fn()
        assert e.value.status == local_map.ERR_INVALID and all(n in e.value.message for n in needles), e.value.message
    nan_T = list(cases.I12)
    nan_T[7] = float("nan")
    refused(lambda: m.points_write(6, [[0, 0, 1]]), "gap")
    refused(lambda: m.points_write(0, [[0, np.inf, 1]]), "p_world")
    refused(lambda: m.keyframe_add(nan_T, [0]), "T_kf_w")
    refused(lambda: m.keyframe_add(cases.I12, [0, 4]), "point_of_slot[1]")
    refused(lambda: m.keyframe_add(cases.I12, [-2]), "point_of_slot[0]")
    refused(lambda: m.keyframe_add(cases.I12, [-1] * (local_map.MAX_SLOTS + 1)), "n_slots")
    refused(lambda: m.keyframe_write(3, cases.I12), "keyframe 3")
    refused(lambda: m.keyframe_write(1, None, 1, [0, 0]), "keyframe 1", "slots")
    refused(lambda: m.keyframe_write(1, nan_T), "keyframe 1", "T_kf_w")
    refused(lambda: foreign.ctx.select(cases.CAM, [(m, cases.I12, 4)]), "desc 0", "map")
    for kw, needle in ((dict(n_local=0), "n_local"), (dict(n_local=65), "n_local"), (dict(boundary=-1), "boundary")):
        refused(lambda: lm_ctx.select(cases.CAM, [(m, cases.I12, 4)], **kw), needle)
    refused(lambda: lm_ctx.select(cases.CAM, [(m, cases.I12, 4), (m, nan_T, 4)]), "desc 1", "T_cur_w")
    refused(lambda: lm_ctx.select(cases.CAM, [(m, cases.I12, 2 * local_map.MAX_SLOTS + 1)], n_local=2), "desc 0", "point_capacity")
    cam = copy.copy(cases.CAM)
    cam.width = 0
    refused(lambda: lm_ctx.select(cam, [(m, cases.I12, 4)]), "camera")
    call = local_map.SelectCall(lm_ctx, cases.CAM, [(m, cases.I12, 4), (foreign, cases.I12, 4)])
    assert call.run_raw() == local_map.ERR_INVALID and "desc 1" in lm_ctx.last_error()
    assert all((a.view(np.uint8) == local_map.FILL).all() for k in call.keep for a in k[2:6])
    assert bytes(call.results) == bytes([local_map.FILL]) * len(bytes(call.results))
    assert lm_ctx.select(cases.CAM, [], 10, 0) == []
    after = m.read()
    assert all(np.array_equal(before[k], after[k]) for k in ("p_world", "bad", "T_kf_w")) and all(np.array_equal(a, b) for a, b in zip(before["slots"], after["slots"]))
    cases.same_answer(lm_ctx.select(cases.CAM, [(m, cases.I12, 8)], 2, 0)[0], dict(cases.expected(c)[0]), "after the refusals")
    foreign.close()
    other.close()
    m.close()


def test_a_map_whose_seen_bitmap_needs_the_large_lds_opt_in(lm_ctx):
    """More than 64 KiB of dynamic LDS is an opt-in of the select kernel: 600 000 points make the seen-bitmap 75 000 bytes. One tiny
    keyframe lists the first, a middle and the last point (the last one twice) and a bad one: the answer is known by hand."""
    P = 600_000
    X = np.zeros((P, 3))
    X[:, 2] = -5.0                                           # behind the camera ...
    X[[0, 300_000, P - 1, P - 2]] = [cases.at_pixel(10, 10), cases.at_pixel(20, 10), cases.at_pixel(30, 10), cases.at_pixel(40, 10)]
    bad = np.zeros(P, np.uint8)
    bad[P - 2] = 1
    m = lm_ctx.new_map()
    m.points_write(0, X[:400_000], bad[:400_000])
    m.points_write(400_000, X[400_000:], bad[400_000:])
    assert m.keyframe_add(cases.pose((0.5, 0, 0)), [P - 1, -1, 0, P - 2, 300_000, P - 1, 5]) == 0
    got = lm_ctx.select(cases.CAM, [(m, cases.I12, 8), (m, cases.pose((0, 0, 100.0)), 8)], 10, 0)
    assert got[0]["kf"] == [0] and got[0]["kf_dist"] == [0.5] and got[0]["point"] == [P - 1, 0, 300_000, 5] and got[0]["point_kf"] == [0, 0, 0, 0]
    assert (got[0]["n_close"], got[0]["n_kf"], got[0]["n_points"], got[0]["overflow"]) == (1, 1, 4, 0)
    assert got[1]["kf"] == [0] and got[1]["point"] == got[0]["point"]
    m.close()


def test_cpp_adapter_and_example_on_the_device(tmp_path):
    """dsdtm_amd/host/example_localmap.cpp: DSDTM::LocalMap over the C ABI, Select against select_local_map_host, and
    UpdateLocalMapOnDevice (with a capacity that is too small at first) — it exits with 0 only when all three agree."""
    import os
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsdtm_amd", "host")
    lib, exe = local_map.lib_path(), str(tmp_path / "example_localmap")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(host, "example_localmap.cpp"), lib,
                    "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "2 local keyframes" in r.stdout and r.stdout.count("the same") == 2 and "TrackFrame takes all 3" in r.stdout, r.stdout


def test_store_to_update_local_map_to_track_frame(gpu_ctx, lm_ctx):
    """LocalMapStore -> Tracker.UpdateLocalMap -> track_frame on the small synthetic search world: the same tracked frame as with
    the lists the restatement builds from the store's mirror."""
    from tests.test_search_gpu import make_world
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    cam, kfs, cur, mps = make_world(21, n_points=700, n_kf=2)
    for k, kf in enumerate(kfs):
        mpts = [None] * kf.n_features
        for mp in mps:
            if k in mp.mObservations:
                mpts[mp.mObservations[k]] = mp
        kf.mvMapPoints = mpts
    store = local_map.LocalMapStore(lm_ctx)
    for kf in kfs:
        store.add_keyframe(kf)
    tr = tracking.Tracker(cam, gpu_ctx, 5, 0, 8)
    T = cur.Get_Pose()
    keyframes, map_points = tr.UpdateLocalMap(store, T)
    want = R.select_local_map(cam, T, store.mirror(), 10, 0)
    assert [store.keyframe_index(k) for k in tr.local_keyframes] == want["kf"] and len(want["kf"]) == 2
    assert [store.point_index(mp) for mp in map_points] == want["point"] and len(want["point"]) > 300
    assert keyframes == kfs
    restated = [store.points[p] for p in want["point"]]
    last = Frame(cam, cur.mvImg_Pyr, T)
    rs = [tracking.track_frame(gpu_ctx, cam, cur.mvImg_Pyr[0], 5, last, T, (5, 0, 8, 15), 0, keyframes, lst) for lst in (map_points, restated)]
    assert np.array_equal(rs[0]["matches"], rs[1]["matches"]) and len(rs[0]["matches"]) > 20 and rs[0]["n_in_grid"] == rs[1]["n_in_grid"] > 100
    assert np.array_equal(rs[0]["T_opt"], rs[1]["T_opt"]) and np.array_equal(rs[0]["T_run"], rs[1]["T_run"])
    ks, ms = tracking.MultiTracker(cam, gpu_ctx, 5, 0, 8).UpdateLocalMaps([store, store], [T, T])
    assert ks == [keyframes, keyframes] and ms == [map_points, map_points]
    for r in rs:
        r["frame"].close()
