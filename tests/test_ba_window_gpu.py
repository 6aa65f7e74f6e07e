"""libdsdtm_amd_mapping.so (include/dsdtm_amd_mapping.h) on the MI355X: dsdtm_mapping_covisibility, dsdtm_mapping_ba_window and
dsdtm_mapping_ba_commit (hand-set outlier flags, poses and points moved by hand in place of the solver) against the restatement
(dsdtm_amd/ba_window_restatement.py) on every case of tests/ba_window_cases.py — lists, counts and flags equal, every copied value
bit-equal, the map after a commit equal to the restated one byte for byte — and the resident map's entries against
libdsdtm_amd_trackmap.so's on the same worlds (one implementation, compiled twice). No tolerance anywhere: every value is a copy."""
import copy

import numpy as np
import pytest

from dsdtm_amd import ba_window, track_map
from dsdtm_amd import track_map_restatement as TR
from tests import ba_window_cases as cases
from tests import track_map_cases
from tests.local_map_cases import CAM, I12

pytestmark = pytest.mark.gpu
INVALID = -2


@pytest.fixture(scope="module")
def mp_ctx():
    ctx = ba_window.MappingContext(0)
    yield ctx
    ctx.close()


def upload(ctx, world):
    m = ctx.new_map()
    m.points_write(0, world["p_world"], world["bad"], world["found"])
    for k in range(len(world["slots"])):
        assert m.keyframe_add(world["T_kf_w"][k], world["slots"][k], world["observes"][k], world["px"][k], world["level"][k], world["bearing"][k]) == k
    return m


def window_call(ctx, maps, windows, room=cases.ROOM):
    return ba_window.WindowCall(ctx, [(maps[w], kf, cov, origin, room["kcap"] if kc is None else kc, room["pcap"] if pc is None else pc,
                                       room["ocap"] if oc is None else oc) for w, kf, cov, origin, kc, pc, oc in windows])


def check_windows(call, got, want, name):
    sums = dict(kf=0, point=0, obs=0)
    for i, (g, w) in enumerate(zip(got, want)):
        cases.same_window(g, w, (name, i))
        p = g["problem"]
        assert (p["keyframe_offset"], p["point_offset"], p["observation_offset"]) == (sums["kf"], sums["point"], sums["obs"]), (name, i, p)
        d = call.descs[i]
        sums["kf"] += d.keyframe_capacity; sums["point"] += d.point_capacity; sums["obs"] += d.observation_capacity
        if w["usable"]:
            assert (p["n_keyframes"], p["n_points"], p["n_observations"]) == (w["n_local"] + w["n_fixed"], w["n_points"], w["n_obs"]), (name, i, p)
            for h, dev in (("h_kf_index", "kf_index"), ("h_point_index", "point_index"), ("h_obs_slot", "obs_slot")):
                assert np.array_equal(g[h], g[dev]), (name, i, h)
            assert np.all(np.diff(g["obs_point"]) >= 0)
        else:
            assert (p["n_keyframes"], p["n_points"], p["n_observations"]) == (0, 0, 0), (name, i, p)


def moved(call, want):
    """In place of the solver: every usable window's poses and points get new values on the device (exact in binary, so that the
    restated commit holds the same bits). Returns the values per window."""
    import torch
    T = call.column("T_c2w").copy()
    X = call.column("points").copy()
    out = []
    for i, w in enumerate(want):
        if not w["usable"]:
            out.append(None)
            continue
        at = call.offsets[i]
        nk, npt = w["n_local"] + w["n_fixed"], w["n_points"]
        T[at["kf"]:at["kf"] + nk, 3] += 0.25 * (i + 1)
        X[at["point"]:at["point"] + npt] += 0.125 * (i + 1)
        out.append((T[at["kf"]:at["kf"] + nk].copy(), X[at["point"]:at["point"] + npt].copy()))
    call.tensors["T_c2w"].copy_(torch.from_numpy(T.reshape(-1).view(np.uint8)))
    call.tensors["points"].copy_(torch.from_numpy(X.reshape(-1).view(np.uint8)))
    torch.cuda.synchronize()
    return out


def outlier_tensor(call, flags):
    import torch
    host = np.full(max(call.total["obs"], 1), 7, np.uint8)
    for i, f in enumerate(flags):
        if f is not None:
            host[call.offsets[i]["obs"]:call.offsets[i]["obs"] + len(f)] = f
    return torch.from_numpy(host).to("cuda:0")


@pytest.mark.parametrize("c", cases.all_cases() + cases.size_cases(), ids=lambda c: c["name"])
def test_every_case_equals_the_restatement(mp_ctx, c):
    import torch
    want = cases.expected(c)
    maps = [upload(mp_ctx, w) for w in c["worlds"]]
    try:
        if c["cov"]:
            got = mp_ctx.covisibility([(maps[w], kf, cap) for w, kf, cap in c["cov"]])
            for q, (g, e, (_, _, cap)) in enumerate(zip(got, want["cov"], c["cov"])):
                for k in ("n_cov", "n_connected", "overflow", "cov_kf", "cov_weight"):
                    assert g[k] == e[k], (c["name"], q, k, g[k], e[k])
                for raw in g["raw"]:                            # behind what the result reports: untouched
                    assert np.all(raw.view(np.uint8)[4 * min(e["n_cov"], cap):] == ba_window.FILL)
        if not c["windows"]:
            return
        call = window_call(mp_ctx, maps, c["windows"], c["room"])
        got = call.run()
        check_windows(call, got, want["windows"], c["name"])
        if c["outliers"] is None:
            return
        bad_capacity = 8 if c["bad_capacity"] is None else c["bad_capacity"]        # (the rule-edge cases turn at most 4 points bad)
        # the commit: the restated one takes the same moved poses and points
        values = moved(call, want["windows"])
        worlds = [copy.deepcopy(w) for w in c["worlds"]]
        restated = []
        for i, w in enumerate(want["windows"]):
            if want["overlap"] or not w["usable"]:
                restated.append(None)
                continue
            m = c["windows"][i][0]
            worlds[m], r = cases.BR.ba_commit(worlds[m], w, values[i][0], values[i][1], want["flags"][i], c["bad_capacity"])
            restated.append(r)
        st, res = call.commit(outlier_tensor(call, want["flags"]), torch.cuda.current_stream().cuda_stream, bad_capacity=bad_capacity)
        if want["overlap"]:
            a, b = want["overlap"]
            assert c["overlap"] == want["overlap"] and st == INVALID and f"windows {a} and {b}" in mp_ctx.last_error(), (st, mp_ctx.last_error())
        else:
            assert st == 0, mp_ctx.last_error()
            for i, (g, e, r) in enumerate(zip(res, want["commits"], restated)):
                if e is None:
                    assert (g["n_outliers"], g["n_bad"], g["overflow_bad"]) == (0, 0, 0)
                    continue
                assert r["n_outliers"] == e["n_outliers"] and r["bad_points"] == e["bad_points"]      # (moving the values changes no bookkeeping)
                for k in ("n_outliers", "n_bad", "overflow_bad", "bad_points"):
                    assert g[k] == e[k], (c["name"], i, k, g[k], e[k])
        for m, w in zip(maps, worlds):                          # (refused: `worlds` are the untouched ones)
            cases.same_world(m.read(), w, c["name"])
    finally:
        for m in maps:
            m.close()


def test_the_map_entries_are_the_trackmap_library_s(mp_ctx):
    """dsdtm_mapping_local and dsdtm_mapping_map_read against dsdtm_trackmap_local and dsdtm_trackmap_map_read on the same world: the
    same bytes (one implementation, compiled into both libraries)."""
    tm_ctx = track_map.TrackMapContext(0)
    try:
        for c in track_map_cases.small_cases():
            a, b = upload(mp_ctx, c["world"]), upload(tm_ctx, c["world"])
            for T, want in zip(c["poses"], track_map_cases.expected(c)):
                ocap = track_map_cases.obs_capacity_of(c, want)
                ga = mp_ctx.local(CAM, [(a, T, c["point_capacity"], ocap)], c["n_local"])[0]
                gb = tm_ctx.local(CAM, [(b, T, c["point_capacity"], ocap)], c["n_local"])[0]
                track_map_cases.same_answer(ga, want, c["name"])
                for k in ga["raw"]:
                    assert ga["raw"][k].tobytes() == gb["raw"][k].tobytes(), (c["name"], k)
            cases.same_world(a.read(), b.read(), c["name"])
            a.close(); b.close()
    finally:
        tm_ctx.close()


def test_a_window_alone_and_as_one_of_eight_gives_the_same_bytes(mp_ctx):
    c = cases.by_name("window_two_windows_on_one_map_and_two_maps")
    maps = [upload(mp_ctx, w) for w in c["worlds"]]
    alone_call = window_call(mp_ctx, maps, c["windows"][:1])
    alone = alone_call.run()[0]
    eight = [c["windows"][i % 3] for i in (1, 2, 1, 2, 2, 0, 1, 2)]
    call = window_call(mp_ctx, maps, eight)
    got = call.run()
    want = cases.expected(c)["windows"]
    check_windows(call, got, [want[i % 3] for i in (1, 2, 1, 2, 2, 0, 1, 2)], "one of eight")
    for k in cases.WINDOW_COLUMNS:
        assert np.asarray(alone[k]).tobytes() == np.asarray(got[5][k]).tobytes(), k
    for f in ba_window.RESULT_FIELDS:
        assert alone[f] == got[5][f], f
    # behind a window's counts nothing was written: the fill bytes stand
    at, w = call.offsets[5], want[0]
    assert np.all(call.column("points")[at["point"] + w["n_points"]:at["point"] + cases.ROOM["pcap"]].view(np.uint8) == ba_window.FILL)
    assert np.all(call.column("obs_slot")[at["obs"] + w["n_obs"]:at["obs"] + cases.ROOM["ocap"]].view(np.uint8) == ba_window.FILL)
    for m in maps:
        m.close()


def test_windows_of_very_different_sizes_in_one_call_equal_each_alone(mp_ctx):
    """window_mixed_call: a 700-entry window, a 5-entry window on a 6-keyframe map and a window on a 66-keyframe map share every launch
    (the grids are sized by the largest; the small ones' extra workgroups must return): each result is byte-equal to the same window
    run alone, and behind each window's counts the fill bytes stand."""
    c = cases.by_name("window_mixed_call")
    want = cases.expected(c)["windows"]
    maps = [upload(mp_ctx, w) for w in c["worlds"]]
    try:
        call = window_call(mp_ctx, maps, c["windows"], c["room"])
        got = call.run()
        check_windows(call, got, want, c["name"])
        cap = dict(kf=c["room"]["kcap"], point=c["room"]["pcap"], obs=c["room"]["ocap"])
        whole = {name: call.column(name) for name, _, _, _ in ba_window.DEVICE_ARRAYS}
        for i, spec in enumerate(c["windows"]):
            alone = window_call(mp_ctx, maps, [spec], c["room"]).run()[0]
            for k in cases.WINDOW_COLUMNS:
                assert np.asarray(alone[k]).tobytes() == np.asarray(got[i][k]).tobytes(), (i, k)
            for f in ba_window.RESULT_FIELDS:
                assert alone[f] == got[i][f], (i, f)
            cnt = dict(kf=want[i]["n_local"] + want[i]["n_fixed"], point=want[i]["n_points"], obs=want[i]["n_obs"])
            for name, _, _, by in ba_window.DEVICE_ARRAYS:
                at = call.offsets[i][by]
                assert np.all(whole[name][at + cnt[by]:at + cap[by]].view(np.uint8) == ba_window.FILL), (i, name)
    finally:
        for m in maps:
            m.close()


def test_local_after_a_commit_sees_moved_points_and_no_bad_ones(mp_ctx):
    import torch
    c = cases.by_name("commit_all_of_them_together")
    want = cases.expected(c)
    m = upload(mp_ctx, c["worlds"][0])
    call = window_call(mp_ctx, [m], c["windows"])
    call.run()
    values = moved(call, want["windows"])
    world, r = cases.BR.ba_commit(c["worlds"][0], want["windows"][0], values[0][0], values[0][1], want["flags"][0])
    st, res = call.commit(outlier_tensor(call, want["flags"]), torch.cuda.current_stream().cuda_stream, bad_capacity=2)
    assert st == 0 and res[0]["n_bad"] == r["n_bad"] == 4 and res[0]["overflow_bad"] == 1 and res[0]["bad_points"] == r["bad_points"][:2]
    T = np.array(I12, np.float64)
    T[3] = -float(c["objects"][0][0][3].centre_x)           # at keyframe 3
    e = TR.track_map_local(CAM, T, world, 4, 0, 4096, None)
    g = mp_ctx.local(CAM, [(m, T, 4096, max(e["n_obs"], 1))], 4)[0]
    track_map_cases.same_answer(g, e, "local after commit")
    assert e["n_points"] > 0 and not set(r["bad_points"]) & set(g["point"])
    stayed = [p for p in want["windows"][0]["point_index"].tolist() if p in g["point"]]
    assert stayed                                           # a moved point that stayed good comes back at its NEW position
    for p in stayed:
        i = want["windows"][0]["point_index"].tolist().index(p)
        assert track_map_cases.same_bits(g["flat"]["pw"][g["point"].index(p)], values[0][1][i])
    m.close()


def test_refused_window_calls_name_the_desc_and_write_nothing(mp_ctx):
    c = cases.by_name("window_first_occurrence_fixed_order_listed_unobserved")
    m = upload(mp_ctx, c["worlds"][0])
    good = (0, 5, [3, 4], -1, None, None, None)
    for bad, needle in (((0, 5, [3, 5], -1, None, None, None), "cov_kf contains kf"), ((0, 5, [3, 3], -1, None, None, None), "repeats"),
                        ((0, 5, [6], -1, None, None, None), "outside the map"), ((0, 6, [], -1, None, None, None), "kf is not a keyframe"),
                        ((0, 5, [3], 9, None, None, None), "origin_kf"), ((0, 5, [3], -1, 81, None, None), "keyframe_capacity")):
        call = window_call(mp_ctx, [m], [good, bad])
        assert call.run_raw() == INVALID and "desc 1" in mp_ctx.last_error() and needle in mp_ctx.last_error(), mp_ctx.last_error()
        for name in call.tensors:
            assert np.all(call.column(name).view(np.uint8) == ba_window.FILL), name
    m.close()


def test_the_chain_window_solve_commit_equals_the_restated_chain(gpu_ctx, mp_ctx):
    """Optimizer.LocalBundleAdjustmentOnDevice — window -> dsdtm_local_ba_batch_device -> commit, the commit enqueued behind the solve
    with no wait in between — against restated window -> dsdtm_local_ba on host arrays -> restated commit, on one world: poses, points,
    outlier flags and the final map are bit-equal (the solver is deterministic and its input columns are copies)."""
    from dsdtm_amd.optimizer import Optimizer, local_bundle_adjustment
    world, kf, cov, delta = cases.chain_world()
    m = upload(mp_ctx, world)
    got = Optimizer.LocalBundleAdjustmentOnDevice(mp_ctx, m, kf, cov, -1, delta, ctx=gpu_ctx, capacities=(16, 128, 512), bad_capacity=64)
    assert got is not None
    win = cases.BR.ba_window(world, kf, cov, -1)
    cases.same_window(got["window"], win, "chain")
    T, X = win["T_c2w"].reshape(-1).copy(), win["points"].reshape(-1).copy()
    out, sm = local_bundle_adjustment(gpu_ctx, T, win["kf_constant"], X, win["obs_kf"], win["obs_point"], win["obs_bearing"], win["obs_level"], delta)
    out = out[:win["n_obs"]]
    after, r = cases.BR.ba_commit(world, win, T.reshape(-1, 12), X.reshape(-1, 3), out)
    n_out, n_bad, good_with_outlier = cases.chain_property(win, out, r)
    print("chain: outliers", n_out, "bad", n_bad, "good points with an outlier", good_with_outlier)
    assert n_out >= 1 and n_bad >= 1 and good_with_outlier >= 1           # (the case must not turn vacuous)
    assert np.array_equal(got["outlier"], out)
    assert track_map_cases.same_bits(got["T_c2w"], T.reshape(-1, 12)) and track_map_cases.same_bits(got["points"], X.reshape(-1, 3))
    for k in ("n_outliers", "n_bad", "overflow_bad", "bad_points"):
        assert got["commit"][k] == r[k], (k, got["commit"][k], r[k])
    assert got["summary"]["n_outliers"] == n_out and got["summary"]["iterations"] == sm["iterations"]
    cases.same_world(m.read(), after, "chain")
    m.close()


def test_refused_covisibility_and_commit_calls_leave_the_map_unchanged(mp_ctx):
    """The host-side checks of the other two entries: DSDTM_ERR_INVALID naming the desc and the field, nothing written."""
    import torch
    c = cases.by_name("commit_one_of_two_point_goes_bad")
    want = cases.expected(c)
    m = upload(mp_ctx, c["worlds"][0])
    for pairs, needle in (([(m, 4, 4)], "desc 0: kf"), ([(m, 0, 4), (m, -1, 4)], "desc 1: kf"), ([(m, 0, -1)], "capacity"), ([(m, 0, 1)] * 1025, "outside 0..1024")):
        with pytest.raises(ba_window.MappingError) as e:
            mp_ctx.covisibility(pairs)
        assert e.value.status == INVALID and needle in e.value.message, e.value.message
    call = window_call(mp_ctx, [m], [c["windows"][0], c["windows"][0]])        # (two windows: the second one's offsets are not 0)
    call.run()
    flags = outlier_tensor(call, [want["flags"][0], want["flags"][0]])
    stream = torch.cuda.current_stream().cuda_stream

    def refused(needle, bad_capacity=8):
        st, _ = call.commit(flags, stream, bad_capacity=bad_capacity)
        assert st == INVALID and needle in mp_ctx.last_error(), (st, mp_ctx.last_error())
        cases.same_world(m.read(), c["worlds"][0], needle)
    refused("bad_capacity", bad_capacity=-1)
    refused("windows 0 and 1")                                                  # (the same window twice overlaps itself)
    call.problems[1].point_offset += 1
    refused("desc 1: problems: the offsets")
    call.problems[1].point_offset -= 1
    call.problems[0].n_points = call.descs[0].point_capacity + 1
    refused("desc 0: problems: a count exceeds")
    call.problems[0].n_points = want["windows"][0]["n_points"]
    call.descs[1].kf = 99
    refused("desc 1: kf is not a keyframe")
    m.close()
