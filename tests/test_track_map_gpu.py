"""dsdtm_trackmap_local and the device-resident track map (include/dsdtm_amd_trackmap.h) on the MI355X against the restatement
(dsdtm_amd/track_map_restatement.py) on the worlds of tests/track_map_cases.py: kf, point, point_kf, counts and flags equal, kf_dist and
every column bit-equal — no tolerance: the selection's arithmetic is correctly rounded on both sides and the flatten only copies.
Then the repeat and the batch (arrival order must not show), the updates with their re-allocations, map_read, the argument checks,
the C++ example and the hand-over into dsdtm_track_frame."""
import copy
import os
import subprocess

import numpy as np
import pytest

from dsdtm_amd import track_map, tracking
from dsdtm_amd import track_map_restatement as TR
from dsdtm_amd.frame import Config, Frame
from tests import track_map_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tm_ctx():
    ctx = track_map.TrackMapContext(0)
    yield ctx
    ctx.close()


def upload(ctx, world, k0=0, k1=None, m=None, piece=None):
    """The world's keyframes [k0, k1) into a device map, each preceded by the points it needs (point indices are the world's)."""
    m = m or ctx.new_map()
    k1 = len(world["slots"]) if k1 is None else k1
    have = m.n_points if hasattr(m, "n_points") else 0
    for k in range(k0, k1):
        need = int(world["slots"][k].max(initial=-1)) + 1
        if k == len(world["slots"]) - 1:
            need = len(world["p_world"])                        # (points that no keyframe lists ride along with the last one)
        step = piece or max(need - have, 1)
        for a in range(have, need, step):
            b = min(a + step, need)
            m.points_write(a, world["p_world"][a:b], world["bad"][a:b], world["found"][a:b])
        have = max(have, need)
        assert m.keyframe_add(world["T_kf_w"][k], world["slots"][k], world["observes"][k], world["px"][k], world["level"][k], world["bearing"][k]) == k
    m.n_points = have
    return m


def sub_world(world, k1):
    """The world as it is after the first k1 keyframes were uploaded."""
    P = max(int(s.max(initial=-1)) for s in world["slots"][:k1]) + 1
    out = {k: (v[:P] if k in ("p_world", "bad", "found") else v[:k1]) for k, v in world.items()}
    return out


def check_guards(got, cap, ocap):
    """Nothing is written past what the call reports: the rest of every output array still holds the fill bytes."""
    m, no, raw = min(got["n_points"], cap), min(got["n_obs"], ocap), got["raw"]
    ends = dict(kf=got["n_kf"], kf_dist=got["n_kf"], point=m, point_kf=m, mp_world=3 * m, mp_found=m, mp_bad=m, obs_offset=m + 1, obs_kf=no, obs_px=2 * no,
                obs_level=no, obs_bearing=3 * no)
    for name, end in ends.items():
        assert (raw[name][end:].view(np.uint8) == track_map.FILL).all(), name


def raw_bytes(ans):
    return b"".join(ans["raw"][name].tobytes() for name, _, _ in track_map.LocalCall.OUT)


@pytest.mark.parametrize("c", cases.all_cases(), ids=lambda c: c["name"])
def test_local_equals_the_restatement(tm_ctx, c):
    m = upload(tm_ctx, c["world"])
    wants = cases.expected(c)
    queries = [(m, T, c["point_capacity"], cases.obs_capacity_of(c, want)) for T, want in zip(c["poses"], wants)]
    singles = []
    for q, (query, want) in enumerate(zip(queries, wants)):
        got = tm_ctx.local(cases.CAM, [query], c["n_local"], 0)[0]
        cases.same_answer(got, want, (c["name"], q))
        check_guards(got, query[2], query[3])
        again = tm_ctx.local(cases.CAM, [query], c["n_local"], 0)[0]
        assert raw_bytes(again) == raw_bytes(got), (c["name"], q, "the same call twice")
        singles.append(got)
    for q, got in enumerate(tm_ctx.local(cases.CAM, queries, c["n_local"], 0)):      # all poses in one call: the bytes of the single calls
        assert raw_bytes(got) == raw_bytes(singles[q]), (c["name"], "batch", q)
    m.close()


def test_two_descs_on_one_map_and_two_maps_in_one_call(tm_ctx):
    a, b = cases.by_name("plain_trajectory"), cases.by_name("observed_from_outside_the_local_set")
    ma, mb = upload(tm_ctx, a["world"]), upload(tm_ctx, b["world"], piece=7)
    plan = [(ma, a, a["poses"][0], 4096, 4096), (mb, b, b["poses"][0], 64, 512), (ma, a, a["poses"][1], 10, 9), (mb, b, cases.I12, 4096, 0),
            (ma, a, a["poses"][0], 0, 16)]
    got = tm_ctx.local(cases.CAM, [(m, T, cap, ocap) for m, _, T, cap, ocap in plan], 3, 0)
    for i, (m, c, T, cap, ocap) in enumerate(plan):
        want = TR.track_map_local(cases.CAM, T, c["world"], 3, 0, cap, ocap)
        cases.same_answer(got[i], want, i)
        check_guards(got[i], cap, ocap)
        assert raw_bytes(tm_ctx.local(cases.CAM, [(m, T, cap, ocap)], 3, 0)[0]) == raw_bytes(got[i]), ("single", i)
    assert got[2]["overflow_points"] == 1 and got[2]["overflow_obs"] == 1 and got[3]["overflow_obs"] == 1 and got[4]["n_obs"] == 0
    ma.close()
    mb.close()


def test_found_write_between_two_calls(tm_ctx):
    c = cases.by_name("found_counts_change")
    w = copy.deepcopy(c["world"])
    m = upload(tm_ctx, w)
    query = [(m, c["poses"][0], 4096, 4096)]
    cases.same_answer(tm_ctx.local(cases.CAM, query, c["n_local"], 0)[0], TR.track_map_local(cases.CAM, c["poses"][0], w, c["n_local"], 0, 4096, 4096), "before")
    idx, val = [p for p, _ in c["found_updates"]], [v for _, v in c["found_updates"]]
    m.found_write(idx, val)
    w["found"][idx] = val
    want = TR.track_map_local(cases.CAM, c["poses"][0], w, c["n_local"], 0, 4096, 4096)
    assert set(idx) & set(want["point"])
    cases.same_answer(tm_ctx.local(cases.CAM, query, c["n_local"], 0)[0], want, "after")
    m.points_write(4, w["p_world"][4:7])                                           # bad and found NULL on a rewrite: unchanged
    assert np.array_equal(m.read()["found"], w["found"]) and np.array_equal(m.read()["bad"], w["bad"])
    for fn, needle in ((lambda: m.found_write([0, 3, 0], [1, 2, 3]), "twice"), (lambda: m.found_write([len(w["found"])], [1]), "index[0]"),
                       (lambda: m.found_write([2, -1], [1, 1]), "index[1]")):
        with pytest.raises(track_map.TrackMapError) as e:
            fn()
        assert e.value.status == track_map.ERR_INVALID and needle in e.value.message, e.value.message
    assert np.array_equal(m.read()["found"], w["found"])
    m.close()


def test_the_map_grows_between_two_calls(tm_ctx):
    """More than 4096 points, 64 keyframes and 16 384 slots: every array of the map is re-allocated between the two calls, and the
    BA-time updates (a pose, a run of slots with their flags) land in the grown arrays."""
    c = cases.by_name("grows_past_the_initial_capacities")
    w, first = copy.deepcopy(c["world"]), c["first_part"]
    m = upload(tm_ctx, w, 0, first)
    part = sub_world(w, first)
    for T in c["poses"]:
        cases.same_answer(tm_ctx.local(cases.CAM, [(m, T, 4096, 20000)], c["n_local"], 0)[0], TR.track_map_local(cases.CAM, T, part, c["n_local"], 0, 4096, 20000), "first part")
    upload(tm_ctx, w, first, None, m, piece=1500)
    for q, (T, want) in enumerate(zip(c["poses"], cases.expected(c))):
        cases.same_answer(tm_ctx.local(cases.CAM, [(m, T, 4096, max(want["n_obs"], 1))], c["n_local"], 0)[0], want, ("whole", q))
    k = cases.expected(c)[0]["kf"][0]
    w["T_kf_w"][k] = cases.pose((-0.31, 0.0, 0.01))
    seen = np.flatnonzero(w["observes"][k][40:90]) + 40
    w["observes"][k][seen[:5]] = 0                            # Erase_Observation alone: the slot stays (the BA quirk)
    w["slots"][k][seen[5:8]], w["observes"][k][seen[5:8]] = -1, 0      # Erase_MapPointMatch as well
    m.keyframe_write(k, w["T_kf_w"][k], 40, w["slots"][k][40:90], w["observes"][k][40:90])
    T = c["poses"][0]
    cases.same_answer(tm_ctx.local(cases.CAM, [(m, T, 4096, 20000)], c["n_local"], 0)[0], TR.track_map_local(cases.CAM, T, w, c["n_local"], 0, 4096, 20000), "after keyframe_write")
    got = m.read()
    for key in ("p_world", "bad", "found", "T_kf_w"):
        assert cases.same_bits(got[key], w[key]), key
    for key in ("slots", "observes", "px", "level", "bearing"):
        assert len(got[key]) == len(w[key]) and all(cases.same_bits(a, np.asarray(b).reshape(a.shape)) for a, b in zip(got[key], w[key])), key
    m.close()


def test_map_read_returns_what_was_written(tm_ctx):
    w = cases.by_name("observation_erased_slot_still_set")["world"]
    m = upload(tm_ctx, w, piece=3)
    got = m.read()
    for key in ("p_world", "bad", "found", "T_kf_w"):
        assert cases.same_bits(got[key], w[key]), key
    for key in ("slots", "observes", "px", "level", "bearing"):
        assert all(cases.same_bits(a, np.asarray(b).reshape(a.shape)) for a, b in zip(got[key], w[key])), key
    assert any((o == 0).any() and ((o == 0) & (s >= 0)).any() for o, s in zip(got["observes"], got["slots"]))      # a set slot that does not observe
    empty = tm_ctx.new_map()
    assert [len(v) for v in empty.read().values()] == [0] * 9
    empty.close()
    m.close()


def test_refused_calls_leave_map_and_outputs_untouched(tm_ctx):
    c = cases.by_name("point_without_observation")
    w = c["world"]
    m, other = upload(tm_ctx, w), track_map.TrackMapContext(0)
    foreign = other.new_map()
    before = m.read()

    def refused(fn, *needles):
        with pytest.raises(track_map.TrackMapError) as e:
            fn()
        assert e.value.status == track_map.ERR_INVALID and all(n in e.value.message for n in needles), e.value.message
    nan_T = list(cases.I12)
    nan_T[7] = float("nan")
    P, col = len(w["p_world"]), lambda n: (np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.zeros((n, 3)))
    refused(lambda: m.points_write(P + 1, [[0, 0, 1]]), "gap")
    refused(lambda: m.points_write(0, [[0, np.inf, 1]]), "p_world")
    refused(lambda: m.keyframe_add(nan_T, [0], [1], *col(1)), "T_kf_w")
    refused(lambda: m.keyframe_add(cases.I12, [0, P], [1, 1], *col(2)), "point_of_slot[1]")
    refused(lambda: m.keyframe_add(cases.I12, [0, -1], [0, 1], *col(2)), "observes[1]", "NULL slot")
    refused(lambda: m.keyframe_add(cases.I12, [0], [2], *col(1)), "observes[0]")
    refused(lambda: m.keyframe_write(2, cases.I12), "keyframe 2")
    refused(lambda: m.keyframe_write(1, None, 5, [0, 0], [1, 0]), "keyframe 1", "slots")
    refused(lambda: m.keyframe_write(1, None, 0, [-1], [1]), "keyframe 1", "observes[0]")
    refused(lambda: m.keyframe_write(1, nan_T), "keyframe 1", "T_kf_w")
    q = (m, cases.I12, 8, 8)
    refused(lambda: other.local(cases.CAM, [q]), "desc 0", "map")
    for kw, needle in ((dict(n_local=0), "n_local"), (dict(n_local=65), "n_local"), (dict(boundary=-1), "boundary")):
        refused(lambda: tm_ctx.local(cases.CAM, [q], **kw), needle)
    refused(lambda: tm_ctx.local(cases.CAM, [q, (m, nan_T, 8, 8)]), "desc 1", "T_cur_w")
    refused(lambda: tm_ctx.local(cases.CAM, [(m, cases.I12, 4097, 8)]), "desc 0", "point_capacity")
    refused(lambda: tm_ctx.local(cases.CAM, [(m, cases.I12, -1, 8)]), "desc 0", "point_capacity")
    refused(lambda: tm_ctx.local(cases.CAM, [q, (m, cases.I12, 8, -1)]), "desc 1", "obs_capacity")
    call = track_map.LocalCall(tm_ctx, cases.CAM, [q])
    call.descs[0].obs_capacity = 2 ** 31 - 1                 # the call's memory limit: refused, not clipped (nothing is enqueued, so the arrays are not touched)
    assert call.run_raw() == track_map.ERR_INVALID and "exceeds" in tm_ctx.last_error()
    cam = copy.copy(cases.CAM)
    cam.width = 0
    refused(lambda: tm_ctx.local(cam, [q]), "camera")
    call = track_map.LocalCall(tm_ctx, cases.CAM, [q, (foreign, cases.I12, 8, 8)])
    assert call.run_raw() == track_map.ERR_INVALID and "desc 1" in tm_ctx.last_error()
    assert all((a.view(np.uint8) == track_map.FILL).all() for k in call.keep for a in k[4].values())
    assert bytes(call.results) == bytes([track_map.FILL]) * len(bytes(call.results))
    call = track_map.LocalCall(tm_ctx, cases.CAM, [q])
    call.descs[0].obs_offset = None
    assert call.run_raw() == track_map.ERR_INVALID and "obs_offset is NULL" in tm_ctx.last_error()
    assert tm_ctx.local(cases.CAM, [], 10, 0) == []
    after = m.read()
    assert all(cases.same_bits(before[k], after[k]) for k in ("p_world", "bad", "found", "T_kf_w"))
    assert all(cases.same_bits(a, b) for k in ("slots", "observes", "px", "level", "bearing") for a, b in zip(before[k], after[k]))
    cases.same_answer(tm_ctx.local(cases.CAM, [(m, cases.I12, 4096, 64)], c["n_local"], 0)[0],
                      TR.track_map_local(cases.CAM, cases.I12, w, c["n_local"], 0, 4096, 64), "after the refusals")
    foreign.close()
    other.close()
    m.close()


def test_cpp_adapter_and_example_on_the_device(tmp_path):
    """dsdtm_amd/host/example_trackmap.cpp: DSDTM::TrackMap over the C ABI, UpdateLocalMapOnDevice (with an observation capacity that is
    too small at first) into a dsdtm_track_desc, against select_local_map_host + flatten_local_map_host — it exits with 0 only when the
    two agree."""
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsdtm_amd", "host")
    lib, exe = track_map.lib_path(), str(tmp_path / "example_trackmap")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(host, "example_trackmap.cpp"), lib,
                    "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "2 local keyframes" in r.stdout and "the same" in r.stdout and "point 9 found 41" in r.stdout, r.stdout


def test_store_to_local_to_track_frame(gpu_ctx, tm_ctx):
    """TrackMapStore -> dsdtm_trackmap_local -> dsdtm_track_frame on the small synthetic search world: the call's dict goes in as
    `flat=` and the tracked frame has the bytes it has when tracking.flatten_local_map walks the objects."""
    from tests.test_search_gpu import make_world
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    cam, kfs, cur, mps = make_world(21, n_points=700, n_kf=2)
    for k, kf in enumerate(kfs):
        mpts = [None] * kf.n_features
        for mp in mps:
            if k in mp.mObservations:
                mpts[mp.mObservations[k]] = mp
        kf.mvMapPoints = mpts
    store = track_map.TrackMapStore(tm_ctx)
    for kf in kfs:
        store.add_keyframe(kf)
    T = cur.Get_Pose()
    r = store.local(cam, T)
    want = TR.track_map_local(cam, T, store.mirror(), 10, 0)
    assert r["kf"] == want["kf"] and r["point"] == want["point"] and len(want["point"]) > 300 and r["n_obs"] == want["n_obs"] > len(want["point"])
    walked = tracking.flatten_local_map(store.keyframes, r["map_points"])
    cases.same_columns(r["flat"], walked, "store against the object walk")
    assert store.capacity_hint == (min(4096, r["n_points"] + r["n_points"] // 4 + 256), r["n_obs"] + r["n_obs"] // 4 + 256)
    store.capacity_hint = (8, 4)                             # remembered capacities that are too small: asked for again, never cut
    again = store.local(cam, T)
    assert again["point"] == r["point"] and not again["overflow_points"] and not again["overflow_obs"]
    cases.same_columns(again["flat"], r["flat"], "after the enlargement")
    mps[r["point"][0]].IncreaseFound(5)                     # a match of the last frame: reported, and in the next answer
    store.update_found([mps[r["point"][0]]])
    r = store.local(cam, T)
    walked = tracking.flatten_local_map(store.keyframes, r["map_points"])
    cases.same_columns(r["flat"], walked, "after IncreaseFound")
    last = Frame(cam, cur.mvImg_Pyr, T)
    rs = [tracking.track_frame(gpu_ctx, cam, cur.mvImg_Pyr[0], 5, last, T, (5, 0, 8, 15), 0, store.keyframes, r["map_points"], flat=flat)
          for flat in (r["flat"], None)]
    assert rs[0]["matches"].tobytes() == rs[1]["matches"].tobytes() and len(rs[0]["matches"]) > 20 and rs[0]["n_in_grid"] == rs[1]["n_in_grid"] > 100
    assert rs[0]["T_opt"].tobytes() == rs[1]["T_opt"].tobytes() and rs[0]["T_run"].tobytes() == rs[1]["T_run"].tobytes()
    assert rs[0]["residual_norm"].tobytes() == rs[1]["residual_norm"].tobytes()
    for x in rs:
        x["frame"].close()
