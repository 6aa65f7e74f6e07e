"""dsdtm_need_keyframes (libdsdtm_amd_keyframe.so: csrc/keyframe.hip, csrc/keyframe_api.cpp) against the restatement dsdtm_amd/keyframe_decision.need_keyframe_reference,
which tests/test_need_keyframe_cpu.py holds to hand-computed answers.

Acceptance: need, reason, rule_mask, n_px, n_depth, svo_kf and undefined EQUAL; the floating quantities within 1e-9 relative
(each is a chain of a few dozen well-conditioned FP64 operations — depths are >= 0.5 m — so rounding is bounded around 1e-13:
1e-9 leaves four orders of margin and still catches a wrong element of the order, a float intermediate or a wrong pose
composition); the two medians bit-equal (kernel and restatement evaluate the transforms in the same order without FMA, and a
selection hands its element through unchanged). Every random case keeps each threshold it does not sit on at least 1e-6
(relative) away from the measured quantity — asserted: a case the restatement places closer is a test bug."""
import copy
import ctypes as C

import numpy as np
import pytest

from dsdtm_amd import capi, synth, tracking
from dsdtm_amd import keyframe_decision as K
from dsdtm_amd.frame import Config
from tests import need_keyframe_cases as cases

pytestmark = pytest.mark.gpu

_REF = {}


def _case(key, build):
    """(case, its reference verdict) — computed once per session, shared, never modified."""
    if key not in _REF:
        c = build()
        r = cases.run_reference(c)
        if not r["undefined"] and key[0] != "exact":
            assert min(cases.margins(c, r)) >= 1e-6, (key, min(cases.margins(c, r)))
        _REF[key] = (c, r)
    return _REF[key]


def _rand(seed, n_cur, n_kf, n_lkf, **kw):
    return _case(("rand", seed, n_cur, n_kf, n_lkf, tuple(sorted(kw.items()))), lambda: cases.random_case(seed, n_cur, n_kf, n_lkf, **kw))


def _run(ctx, cs, params=None):
    return capi.need_keyframes(ctx, cases.CAM, params or cs[0]["params"], [cases.desc_of(c) for c in cs])


@pytest.mark.parametrize("n_cur", [1, 2, 63, 64, 65, 200, 4096])
@pytest.mark.parametrize("depth", ["positive", "negative", "mixed", "equal", "duplicates"])
def test_scene_depth_shapes(gpu_ctx, n_cur, depth):
    c, want = _rand(11 + n_cur, n_cur, 40, 3, depth=depth, bad="some" if n_cur > 2 else "none", fire=2)
    got = _run(gpu_ctx, [c])[0]
    cases.assert_same_verdict(got, want, (n_cur, depth))
    assert got["n_depth"] == len(want["depths"]) and (depth != "negative" or got["median_depth"] < 0)


@pytest.mark.parametrize("n_kf", [0, 30, 31, 32, 300])
@pytest.mark.parametrize("bad", ["none", "some", "all"])
def test_pixel_displacement_shapes(gpu_ctx, n_kf, bad):
    c, want = _rand(23 + n_kf, 50, n_kf, 2, bad=bad, motion=0.05)
    got = _run(gpu_ctx, [c])[0]
    cases.assert_same_verdict(got, want, (n_kf, bad))
    assert got["n_px"] == (0 if bad == "all" else min(31, n_kf) if bad == "none" else want["n_px"])


@pytest.mark.parametrize("n_lkf,fire", [(0, None), (1, 0), (1, None), (10, 9), (10, 0), (64, 63), (64, 0), (64, None)])
def test_local_keyframe_walk(gpu_ctx, n_lkf, fire):
    c, want = _rand(37 + n_lkf, 120, 60, n_lkf, fire=fire)
    assert want["svo_kf"] == (-1 if fire is None else fire)          # (the restatement, on the CPU: the case is what it says)
    cases.assert_same_verdict(_run(gpu_ctx, [c])[0], want, (n_lkf, fire))


@pytest.mark.parametrize("name", sorted(cases.EXACT))
def test_exact_threshold_cases_on_the_device(gpu_ctx, name):
    c, want = _case(("exact", name), cases.EXACT[name])
    cases.assert_same_verdict(_run(gpu_ctx, [c])[0], want, name)
    if name == "k2_31_stop":
        for samples in (30, 40, 64, 1):
            c2 = copy.deepcopy(c)
            c2["params"].px_samples = samples
            cases.assert_same_verdict(_run(gpu_ctx, [c2])[0], cases.run_reference(c2), (name, samples))


def _mixed_batch(n):
    shapes = [(1, 0, 0), (2, 30, 1), (63, 31, 10), (64, 32, 64), (65, 300, 10), (200, 300, 10), (0, 33, 2), (130, 64, 5)]
    depths = ["positive", "negative", "mixed", "equal", "duplicates"]
    out = []
    for t in range(n):
        a, b, l = shapes[t % len(shapes)]
        out.append(_rand(500 + t % 48, a, b, l, depth=depths[t % 5], bad=("none", "some")[t % 2], fire=(l - 1 if l and t % 3 else None),
                         n_valid=(100, 40)[t % 7 == 0]))
    return out


@pytest.mark.parametrize("n", [1, 3, 1024])
def test_batches_of_mixed_shapes(gpu_ctx, n):
    """No tracker reads a neighbour's data: every verdict of the batch equals the restatement of its own tracker."""
    batch = _mixed_batch(n)
    got = _run(gpu_ctx, [c for c, _ in batch])
    assert len(got) == n
    for t, (g, (_, want)) in enumerate(zip(got, batch)):
        cases.assert_same_verdict(g, want, ("batch", n, t))
    assert len({(g["rule_mask"], g["n_px"], g["n_depth"]) for g in got}) >= min(n, 3)


def test_one_large_tracker_among_small_ones(gpu_ctx):
    batch = [_rand(71, 4096, 300, 64, depth="mixed", fire=63), _rand(72, 1, 1, 1, fire=0), _rand(73, 4096, 4096, 10, bad="some", fire=None)]
    for g, (_, want) in zip(_run(gpu_ctx, [c for c, _ in batch]), batch):
        cases.assert_same_verdict(g, want, "large")


def test_a_point_at_the_camera_centre_is_undefined_and_harms_no_neighbour(gpu_ctx):
    a, wa = _rand(81, 65, 40, 3, fire=1)
    # identity rotation, so that the camera centre -t and its depth 0 are exact: the projection there is 0 / 0
    pts = [[(i % 7 - 3) / 8.0, (i % 5 - 2) / 8.0, 1.0 + i / 16.0] for i in range(40)]
    b = cases.make(T_cur=cases.pose(0.25, -0.5, 0.125), T_kf=cases.pose(0.25, -0.5, 0.0625), kf_p=pts, cur_p=pts, lkf=[[1.0, 1.0, 1.0]])
    b["kf_p"][5] = (-0.25, 0.5, -0.125)
    b["cur_p"][7] = (-0.25, 0.5, -0.125)
    c, wc = _rand(83, 200, 300, 10, fire=9)
    assert cases.run_reference(b)["undefined"] == 1
    got = _run(gpu_ctx, [a, b, c])                                      # DSDTM_OK (a failure raises)
    assert got[1]["undefined"] == 1
    solo_a, solo_c = _run(gpu_ctx, [a])[0], _run(gpu_ctx, [c])[0]
    assert got[0] == solo_a and got[2] == solo_c
    cases.assert_same_verdict(got[0], wa, "beside undefined")
    cases.assert_same_verdict(got[2], wc, "beside undefined")


def test_single_entry_equals_the_batch_entry_with_one_tracker(gpu_ctx):
    c, want = _rand(91, 200, 300, 10, fire=4)
    one = capi.need_keyframe(gpu_ctx, cases.CAM, c["params"], cases.desc_of(c))
    assert one == _run(gpu_ctx, [c])[0]
    cases.assert_same_verdict(one, want, "single")
    assert capi.need_keyframes(gpu_ctx, cases.CAM, None, []) == []
    kc = capi.keyframe_context_of(gpu_ctx)
    assert kc.lib.dsdtm_need_keyframes(kc.handle, C.byref(capi.camera_struct(cases.CAM)), C.byref(capi.keyframe_params_struct()),
                                       0, None, None) == capi.OK


def test_invalid_arguments_leave_the_verdicts_untouched(gpu_ctx):
    good = [_rand(500 + t, 20, 35, 3)[0] for t in range(3)]

    def refused(mutate, needle, params=None):
        cs = copy.deepcopy(good)
        call = capi.KeyframeCall(gpu_ctx, cases.CAM, params, [cases.desc_of(c) for c in cs])
        mutate(call)
        call.verdicts.view(np.uint8)[:] = 0xA5
        assert call.run_raw() == capi.ERR_INVALID, needle
        assert np.all(call.verdicts.view(np.uint8) == 0xA5), needle
        msg = capi.keyframe_context_of(gpu_ctx).last_error()
        assert needle in msg, (needle, msg)

    nan = np.array([np.nan])
    refused(lambda k: setattr(k.descs[1], "n_cur_points", capi.KF_MAX_POINTS + 1), "tracker 1: n_cur_points")
    refused(lambda k: setattr(k.descs[2], "n_kf_points", capi.KF_MAX_POINTS + 1), "tracker 2: n_kf_points")
    refused(lambda k: setattr(k.descs[1], "n_local_kf", capi.KF_MAX_LOCAL_KF + 1), "tracker 1: n_local_kf")
    refused(lambda k: setattr(k.descs[1], "cur_p_world", None), "tracker 1: cur_p_world")
    refused(lambda k: setattr(k.descs[0], "kf_p_world", None), "tracker 0: kf_p_world")
    refused(lambda k: setattr(k.descs[2], "local_kf_centre", None), "tracker 2: local_kf_centre")
    refused(lambda k: setattr(k.descs[1], "T_cur_w", None), "tracker 1: T_cur_w")
    refused(lambda k: setattr(k.descs[1], "T_kf_w", None), "tracker 1: T_kf_w")
    refused(lambda k: None, "px_samples", K.KeyframeParams(px_samples=0))
    refused(lambda k: None, "px_samples", K.KeyframeParams(px_samples=65))

    def poke(field, tracker):
        def f(k):
            arr = next(a for a in k._keep if a.size and a.ctypes.data == getattr(k.descs[tracker], field))
            arr.reshape(-1)[arr.size // 2] = np.inf if field == "T_kf_w" else nan[0]
        return f
    for field in ("T_cur_w", "T_kf_w", "cur_p_world", "kf_p_world", "local_kf_centre"):
        refused(poke(field, 1), f"tracker 1: {field}")
    # n over its limit (the descriptors are never read)
    call = capi.KeyframeCall(gpu_ctx, cases.CAM, None, [cases.desc_of(c) for c in good])
    call.verdicts.view(np.uint8)[:] = 0xA5
    kc = capi.keyframe_context_of(gpu_ctx)
    assert kc.lib.dsdtm_need_keyframes(kc.handle, C.byref(call.cs), C.byref(call.prm), capi.TRACK_FRAMES_MAX + 1, call.descs,
                                       call.verdicts.ctypes.data) == capi.ERR_INVALID
    assert np.all(call.verdicts.view(np.uint8) == 0xA5)
    cases.assert_same_verdict(call.run()[0], cases.run_reference(good[0]), "after the refusals")


def test_host_function_agrees_with_the_device(gpu_ctx, tmp_path):
    """need_keyframe_host (dsdtm_host.hpp, no device call) and dsdtm_need_keyframe on the same trackers, through a compiled
    driver that prints both with 17 digits."""
    batch = [_case(("exact", n), cases.EXACT[n]) for n in sorted(cases.EXACT)] + _mixed_batch(16) + \
        [_rand(71, 4096, 300, 64, depth="mixed", fire=63)]
    res = cases.run_driver(tmp_path, [c for c, _ in batch])
    assert len(res["host"]) == len(res["device"]) == len(batch)
    for t, (h, d, (_, want)) in enumerate(zip(res["host"], res["device"], batch)):
        cases.assert_same_verdict(h, d, ("host vs device", t))
        cases.assert_same_verdict(d, want, ("device vs restatement", t))


def test_multitracker_need_keyframes_end_to_end(gpu_ctx):
    """Three sequences, four steps on synth worlds: MultiTracker.NeedKeyframes after each step equals the restatement applied to
    the same Frame / KeyFrame objects (and Tracker.NeedKeyframe on one of them), and the camera moves far enough that a tracker
    flips from 0 to 1 — checked with the restatement, on the CPU. TrackFrames' own results are not touched by the call."""
    from tests.test_search_gpu import make_world
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    n_seq, n_steps, n_kf = 3, 4, 2
    step = np.array([0.010, 0.004, -0.006, 0.003, -0.002, 0.004])
    worlds = []
    for s in range(n_seq):
        cam, kfs, _, mps = make_world(300 + s, n_points=700, n_kf=n_kf)
        for k, kf in enumerate(kfs):
            mpts = [None] * kf.n_features
            for mp in mps:
                if k in mp.mObservations:
                    mpts[mp.mObservations[k]] = mp
            kf.mvMapPoints = mpts
            kf.p_world = np.array([m_.mPose if m_ is not None else np.zeros(3) for m_ in mpts])
            kf.initial = np.array([1 if m_ is not None else 0 for m_ in mpts], np.uint8)
        tex = synth.make_texture(cam.height, cam.width, 300 + s)
        T0 = np.vstack([kfs[n_kf - 1].Get_Pose(), [0, 0, 0, 1]])
        imgs = [synth.warp_plane(tex, cam, synth.se3_exp((k + 1) * (1.0 + 0.25 * s) * step) @ T0, 2.0) for k in range(n_steps)]
        worlds.append((cam, kfs, mps, imgs))
    cam = worlds[0][0]
    # K3 alone decides here: the true translation grows by ~0.0125 m (x 1, 1.25, 1.5) per step and crosses 0.03 m on the way;
    # K1's window is emptied (the count of matches is the tracker's business, not this test's)
    prm = K.KeyframeParams(min_valid=1, max_valid=0, min_rot=1.0, min_trans=0.03)
    mt = tracking.MultiTracker(cam, ctx=gpu_ctx, max_level=5, min_level=0, max_iters=8, min_tracked=20)
    lasts = [w[1][n_kf - 1] for w in worlds]
    last_kfs = [w[1][n_kf - 1] for w in worlds]
    needs = []
    for k in range(n_steps):
        out = mt.TrackFrames([w[3][k] for w in worlds], lasts, [w[1] for w in worlds], [w[2] for w in worlds])
        curs = [o[0] for o in out]
        before = [(c.Get_Pose().copy(), o[1], len(o[2])) for c, o in zip(curs, out)]
        got = mt.NeedKeyframes(curs, last_kfs, [w[1] for w in worlds], prm)
        for s in range(n_seq):
            d = tracking.keyframe_desc(curs[s], last_kfs[s], worlds[s][1])
            assert d["n_valid"] == len(out[s][2]) and len(d["kf_p_world"]) > 100 and len(d["local_kf_centre"]) == n_kf
            want = K.need_keyframe_reference(cam, d["T_cur_w"], d["T_kf_w"], d["n_valid"], d["cur_p_world"], d["cur_bad"], d["kf_p_world"],
                                             d["kf_bad"], d["local_kf_centre"], prm)
            cases.assert_same_verdict(got[s], want, (s, k))
            assert abs(want["trans"] - prm.min_trans) > 1e-6 * prm.min_trans
            assert np.array_equal(curs[s].Get_Pose(), before[s][0]) and (out[s][1], len(out[s][2])) == before[s][1:]
        assert mt.t.NeedKeyframe(curs[0], last_kfs[0], worlds[0][1], prm) == got[0]
        needs.append([g["need"] for g in got])
        lasts = curs
    flips = [s for s in range(n_seq) if needs[0][s] == 0 and needs[-1][s] == 1]
    assert flips, needs
