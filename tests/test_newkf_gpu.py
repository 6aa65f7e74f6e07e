"""dsdtm_newkf_make / dsdtm_newkf_make_batch (libdsdtm_amd_newkf.so, csrc/newkf.hip) on the MI355X against the restatement
(dsdtm_amd/keyframe_creation_restatement.py): every case of tests/newkf_cases.py bit-equal with the cells, the depth image and the
dynamic mask in host memory, in device memory and in pinned memory; batches against their single calls, with a tracker at K1 and one
at overflow among them; the walk's worst case (4096 candidates, no cap); and the chain dsdtm_detect_cells_frame + dsdtm_newkf_make
against Feature_detector.detect + DeviceFrame.lift on a synthetic texture."""
import time

import numpy as np
import pytest

from dsdtm_amd import capi, synth
from dsdtm_amd import keyframe_creation as kc
from dsdtm_amd import keyframe_creation_restatement as R
from tests import newkf_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = kc.NewKeyframeContext(0)
    yield c
    c.close()


def _device(a, dt, pinned=False):
    """A numpy array as a DeviceArray in device (or pinned host) memory; u16 travels as i16 bits."""
    import torch
    a = np.ascontiguousarray(a, dt)
    t = torch.from_numpy(a.view(np.int16) if dt == np.uint16 else a)
    t = t.pin_memory() if pinned else t.cuda()
    torch.cuda.synchronize()
    return kc.DeviceArray(t.data_ptr(), a.shape[1] if a.ndim == 2 else 0, t)


def placed(inp, where):
    """The input with its three image-like arrays in `where`: "host", "device" or "pinned"."""
    if where == "host":
        return inp
    pin = where == "pinned"
    d = dict(inp.__dict__)
    for name, dt in (("cell_score", np.float32), ("cell_x", np.int32), ("cell_y", np.int32), ("cell_level", np.int32), ("depth", np.uint16)):
        d[name] = _device(d[name], dt, pin)
    if inp.dyn_mask is not None:
        d["dyn_mask"] = _device(inp.dyn_mask, np.uint8, pin)
    return R.NewKeyframeInput(**d)


@pytest.mark.parametrize("where", ["host", "device", "pinned"])
@pytest.mark.parametrize("c", cases.all_cases(), ids=lambda c: c["name"])
def test_every_case_is_bit_equal_to_the_restatement(ctx, c, where):
    got = ctx.make(cases.CAM, c["prm"], placed(c["inp"], where))
    assert got["overflow"] == 0
    cases.assert_same(got, cases.answers()[c["name"]], (c["name"], where))
    assert not got["new_bad"].any()
    # nothing behind the counts was written
    raw = got["raw"]
    assert (raw["point_of_slot"].view(np.uint8)[4 * got["n_slots"]:] == kc.FILL).all() and (raw["new_p_world"].view(np.uint8).reshape(-1)[24 * got["n_new_points"]:] == kc.FILL).all()


def test_mixed_memory_kinds_in_one_call(ctx):
    """Each pointer's kind is found on its own: the cells on the device, the depth pageable, the mask pinned."""
    c = [c for c in cases.all_cases() if c["name"] == "dyn_mask_with_existing"][0]
    d = dict(c["inp"].__dict__)
    d["cell_x"], d["cell_level"] = _device(d["cell_x"], np.int32), _device(d["cell_level"], np.int32)
    d["dyn_mask"] = _device(d["dyn_mask"], np.uint8, pinned=True)
    cases.assert_same(ctx.make(cases.CAM, c["prm"], R.NewKeyframeInput(**d)), cases.answers()[c["name"]], "mixed")


def batch_inputs(n):
    """n trackers of one shape and differing n_existing (some at or over the cap: K1)."""
    prm = cases.params(**cases.RAGGED, max_fts=40, min_dist=6)
    inputs = []
    for t in range(n):
        rng = np.random.default_rng(100 + t)
        s, x, y, l = cases.random_cells(rng, prm)
        first = 10 * t
        inp = R.NewKeyframeInput(s, x, y, l, cases.random_depth(rng, prm), 5000.0, cases.pose(rng), first,
                                 **cases.random_existing(rng, prm, 40 + t % 7 if t % 3 == 2 else (13 * t + 3) % 40, first))
        if t % 3 == 1:
            inp.dyn_mask = rng.choice(np.asarray([0, 200, 201], np.uint8), (prm.height, prm.width))
        inputs.append(inp)
    return prm, inputs


@pytest.mark.parametrize("n", [1, 3, 65])
def test_batch_is_bit_equal_to_the_single_calls(ctx, n):
    prm, inputs = batch_inputs(n)
    singles = [ctx.make(cases.CAM, prm, i) for i in inputs]
    assert n < 3 or any(i.n_existing >= prm.max_fts for i in inputs)              # a tracker at K1
    # one tracker gets capacities that do not fit: the others are untouched by that
    over = min(1, n - 1) if n > 1 else -1             # (n = 1: the only tracker is held to its single call; its overflow is the cases')
    caps = [None] * n
    G = prm.grid_cols * prm.grid_rows
    for t, i in enumerate(inputs):
        caps[t] = (i.n_existing + G, i.n_existing + G)
    if over >= 0:
        assert singles[over]["n_new"] > 0
        caps[over] = (inputs[over].n_existing, 0)
    got = ctx.make_batch(cases.CAM, prm, inputs, caps)
    for t in range(n):
        if t == over:
            assert got[t]["overflow"] == 1 and all(got[t][k] == singles[t][k] for k in ("n_new", "n_slots", "n_new_points"))
            assert (got[t]["raw"]["point_of_slot"].view(np.uint8) == kc.FILL).all() and (got[t]["raw"]["new_p_world"].view(np.uint8) == kc.FILL).all()
            continue
        assert got[t]["overflow"] == 0
        cases.assert_same(got[t], singles[t], ("batch", n, t))
        cases.assert_same(got[t], R.create_keyframe(cases.CAM, prm, inputs[t]), ("batch against the restatement", n, t))
        if inputs[t].n_existing >= prm.max_fts:
            assert got[t]["n_new"] == 0 and got[t]["n_slots"] == inputs[t].n_existing


def test_worst_case_of_the_walk(ctx):
    """G = 4096 with every cell above the floor and no cap in reach: 4096 candidates, thousands accepted."""
    prm = R.NewKeyframeParams(1024, 1024, 16, 64, 64, 100000, 8, 20.0)
    rng = np.random.default_rng(4096)
    s, x, y, l = cases.random_cells(rng, prm, scores=tuple(np.linspace(21.0, 500.0, 700)))
    inp = R.NewKeyframeInput(s, x, y, l, cases.random_depth(rng, prm), 5000.0, cases.pose(rng), 7, **cases.random_existing(rng, prm, 50, 7))
    want = R.create_keyframe(cases.CAM, prm, inp)
    assert (s > 20).all() and want["n_new"] > 1500
    ctx.make(cases.CAM, prm, inp)                                                  # (the staging blocks grow here)
    t0 = time.perf_counter()
    got = ctx.make(cases.CAM, prm, inp)
    dt = time.perf_counter() - t0
    print(f"worst case: {want['n_new']} accepted of 4096 candidates, {dt * 1e3:.2f} ms per call")
    cases.assert_same(got, want, "worst case")
    assert dt < 2.0


def test_refusals_leave_the_results_untouched(ctx):
    c = cases.all_cases()[0]
    bad = R.NewKeyframeInput(**{**c["inp"].__dict__, "T_c2w": np.full(12, np.nan)})
    call = kc.MakeCall(ctx, cases.CAM, c["prm"], [c["inp"], bad])
    assert call.run_raw() == kc.ERR_INVALID and "tracker 1: T_c2w" in ctx.last_error()
    for o, r in zip(call.out, call.results):
        assert all((a.view(np.uint8) == kc.FILL).all() for a in o.values()) and r.n_slots == 0
    lv = c["inp"].level.copy(); lv[0] = 16
    with pytest.raises(kc.NewKeyframeError, match="tracker 0: level outside 0..15"):
        ctx.make(cases.CAM, c["prm"], R.NewKeyframeInput(**{**c["inp"].__dict__, "level": lv}))
    cx = c["inp"].cell_x.copy(); cx[3] = -1
    with pytest.raises(kc.NewKeyframeError, match="cell_x is negative"):
        ctx.make(cases.CAM, c["prm"], R.NewKeyframeInput(**{**c["inp"].__dict__, "cell_x": cx}))
    # the same cells in device memory cannot be checked: the kernel skips the corner
    got = ctx.make(cases.CAM, c["prm"], R.NewKeyframeInput(**{**c["inp"].__dict__, "cell_x": _device(cx, np.int32)}))
    s = c["inp"].cell_score.copy(); s[3] = 0
    cases.assert_same(got, R.create_keyframe(cases.CAM, c["prm"], R.NewKeyframeInput(**{**c["inp"].__dict__, "cell_score": s})), "skipped")
    with pytest.raises(kc.NewKeyframeError, match="slot_capacity below n_existing"):
        ctx.make(cases.CAM, c["prm"], c["inp"], capacity=(c["inp"].n_existing - 1, 10))
    cases.assert_same(ctx.make(cases.CAM, c["prm"], c["inp"]), cases.answers()[c["name"]], "the context is usable afterwards")


def test_detect_cells_then_make_equals_detect_then_lift():
    """End to end on a synthetic texture: Feature_detector.detect (the host walk over dsdtm_detect_cells_frame's cells) and
    DeviceFrame.lift give the features and points that dsdtm_detect_cells_frame + dsdtm_newkf_make give."""
    from dsdtm_amd.feature_detection import Feature_detector
    from dsdtm_amd.frame import Config, Frame
    gpu = capi.default_context(0)
    w, h = 640, 480
    img = np.clip(np.rint(synth.make_texture(h, w, 99)), 0, 255).astype(np.uint8)
    rng = np.random.default_rng(5)
    depth = cases.random_depth(rng, R.NewKeyframeParams(w, h, 1, 1, 1, 1, 1), zeros=0.3)
    cam = synth.Camera.tum(w, h)
    det = Feature_detector(w, h, ctx=gpu)
    fr = Frame(cam, synth.build_pyramid(img, 5))
    fr._device_frame = capi.DeviceFrame.prefetch(gpu, img, 5, depth, 5000.0).wait()
    ne = 60
    ex = np.stack([rng.uniform(20, 620, ne), rng.uniform(20, 460, ne)], 1).astype(np.float32)
    has = (rng.random(ne) < 0.7).astype(np.uint8)               # Feature_detector.detect masks around frame.initial
    b = rng.normal(size=(ne, 3))
    fr.set_features(ex, b, np.zeros((ne, 3)), has)
    T = cases.pose(rng)
    det.Set_ExistingFeatures(ex)
    s, x, y, l = (a.copy() for a in det.detect_cells(fr, 5.0))
    n_new = det.detect(fr, 5.0)
    assert 20 < n_new and fr.n_features == ne + n_new
    lifted = np.flatnonzero(np.concatenate([has == 0, np.ones(n_new, bool)]))
    want_d, want_p = fr._device_frame.lift(cam, T, fr.px[lifted])
    prm = R.NewKeyframeParams(w, h, det.mCell_size, det.mGrid_cols, det.mGrid_rows, det.mMax_fts, int(Config.Get("Camera.Min_dist")), 20.0)
    inp = R.NewKeyframeInput(s, x, y, l, depth, 5000.0, T, 500, px_xy=ex, level=np.zeros(ne, np.int32), bearing=b, has_point=has, initial=has,
                             point_index=np.where(has, np.arange(ne), -1).astype(np.int32))
    c = kc.NewKeyframeContext(0)
    got = c.make(cam, prm, inp)
    c.close()
    fr._device_frame.close()
    assert got["n_new"] == n_new and np.array_equal(got["px_xy"], fr.px) and np.array_equal(got["level"][ne:], fr.level[ne:])
    assert got["depth_of_slot"][lifted].tobytes() == want_d.tobytes() and (got["depth_of_slot"][:ne][has == 1] == -1).all()
    assert got["new_p_world"].tobytes() == want_p[want_d >= 0].tobytes() and got["n_new_points"] == int((want_d >= 0).sum()) > 20
    cases.assert_same(got, R.create_keyframe((cam.fx, cam.fy, cam.cx, cam.cy), prm, inp), "end to end against the restatement")


def test_tracker_craete_keyframe_writes_the_map_and_the_covisibility():
    """Tracker.CreateInitialMapRGBD, then Tracker.CraeteKeyframe on a frame that carries some of the first keyframe's points: the map
    read back (map_read) equals the map built from the restated columns and the store's mirror of the objects, the frame object has
    the new features and points, and dsdtm_mapping_covisibility of the new keyframe equals the restated KeyFrame::UpdateConnection
    (ba_window_restatement.update_connection, which update_connection_host is held to bit for bit in tests/test_ba_window_cpu.py)."""
    from dsdtm_amd import ba_window, ba_window_restatement as BR, track_map, tracking
    from dsdtm_amd.feature_detection import Feature_detector
    from dsdtm_amd.frame import Config, Frame
    gpu = capi.default_context(0)
    w, h = 640, 480
    img = np.clip(np.rint(synth.make_texture(h, w, 99)), 0, 255).astype(np.uint8)
    pyr = synth.build_pyramid(img, 5)
    rng = np.random.default_rng(21)
    depth = cases.random_depth(rng, R.NewKeyframeParams(w, h, 1, 1, 1, 1, 1), zeros=0.2)
    cam = synth.Camera.tum(w, h)
    camt = (cam.fx, cam.fy, cam.cx, cam.cy)
    det = Feature_detector(w, h, ctx=gpu)
    prm = R.NewKeyframeParams(w, h, det.mCell_size, det.mGrid_cols, det.mGrid_rows, det.mMax_fts, int(Config.Get("Camera.Min_dist")), 20.0)
    mctx = ba_window.MappingContext(0)
    store = track_map.TrackMapStore(mctx)
    trk = tracking.Tracker(cam, gpu)

    def restated(fr, first):
        ne = fr.n_features
        mps = list(getattr(fr, "mvMapPoints", [None] * ne))
        det.Set_ExistingFeatures(fr.px)
        s, x, y, l = (a.copy() for a in det.detect_cells(fr, 5.0))
        det.ResetGrid()
        inp = R.NewKeyframeInput(s, x, y, l, depth, 5000.0, fr.Get_Pose().reshape(12), first, px_xy=fr.px.copy(), level=fr.level.copy(),
                                 bearing=fr.bearing.copy(), has_point=np.array([m is not None for m in mps], np.uint8), initial=fr.initial.copy(),
                                 point_index=np.array([-1 if m is None else store.point_index(m) for m in mps], np.int32))
        return R.create_keyframe(camt, prm, inp)
    T0, T1 = cases.pose(rng), cases.pose(rng)
    f0 = Frame(cam, pyr, T0.reshape(3, 4))
    want0 = restated(f0, 0)
    a0 = trk.CreateInitialMapRGBD(store, depth, f0)
    assert a0 is not None and a0["kf"] == 0 and a0["n_new"] == want0["n_new"] > 100 and len(store.points) == want0["n_new_points"] >= 100
    assert f0.n_features == want0["n_slots"] and np.array_equal(f0.px, want0["px_xy"]) and a0["cov"]["n_cov"] == 0
    # the next keyframe's frame: 40 features of keyframe 0 that have a point (initial, as SearchLocalPoints leaves them) and 6 tracked
    # features without one
    kf0 = a0["keyframe"]
    have = [i for i, m in enumerate(kf0.mvMapPoints) if m is not None][:40]
    f1 = Frame(cam, pyr, T1.reshape(3, 4))
    extra = np.stack([rng.uniform(30, 600, 6), rng.uniform(30, 440, 6)], 1).astype(np.float32)
    px1 = np.concatenate([kf0.px[have], extra])
    b1 = np.concatenate([kf0.bearing[have], np.tile([0.0, 0.0, 1.0], (6, 1))])
    f1.set_features(px1, b1, np.concatenate([[kf0.mvMapPoints[i].Get_Pose() for i in have], np.zeros((6, 3))]),
                    np.concatenate([np.ones(40, np.uint8), np.zeros(6, np.uint8)]), np.concatenate([kf0.level[have], np.zeros(6, np.int32)]))
    f1.mvMapPoints = [kf0.mvMapPoints[i] for i in have] + [None] * 6
    P0 = len(store.points)
    want1 = restated(f1, P0)
    a1 = trk.CraeteKeyframe(store, depth, cur=f1)
    assert a1["kf"] == 1 and a1["n_new"] == want1["n_new"] > 20 and len(a1["new_points"]) == want1["n_new_points"] > 20
    # the frame object: the new features, and a point for every lifted feature
    assert f1.n_features == want1["n_slots"] and np.array_equal(f1.px, want1["px_xy"]) and np.array_equal(f1.level, want1["level"])
    assert f1.bearing.tobytes() == want1["bearing"].tobytes() and [m is not None for m in f1.mvMapPoints] == (want1["point_of_slot"] >= 0).tolist()
    assert [store.point_index(m) for m in f1.mvMapPoints if m is not None] == want1["point_of_slot"][want1["point_of_slot"] >= 0].tolist()
    # the map: read back == built from the restated columns == the objects' mirror
    want = dict(p_world=np.concatenate([want0["new_p_world"], want1["new_p_world"]]), T_kf_w=np.stack([T0, T1]),
                slots=[want0["point_of_slot"], want1["point_of_slot"]], observes=[want0["observes"], want1["observes"]],
                px=[want0["px_xy"], want1["px_xy"]], level=[want0["level"], want1["level"]], bearing=[want0["bearing"], want1["bearing"]])
    got, mirror = store.map.read(), store.mirror()
    for world in (got, mirror):
        assert world["p_world"].tobytes() == want["p_world"].tobytes() and not world["bad"].any() and not world["found"].any()
        assert np.asarray(world["T_kf_w"]).reshape(2, 12).tobytes() == want["T_kf_w"].tobytes()
        for name in ("slots", "observes", "px", "level", "bearing"):
            for k in range(2):
                a, b = np.asarray(world[name][k]), np.asarray(want[name][k])
                assert a.shape == b.shape and a.tobytes() == b.astype(a.dtype).tobytes(), (name, k)
    # KeyFrame::UpdateConnection of the new keyframe
    cov = BR.update_connection(dict(got), 1)
    assert cov["n_cov"] == 1 and cov["cov_kf"] == [0] and cov["cov_weight"] == [40]
    assert {k: a1["cov"][k] for k in ("n_cov", "n_connected", "overflow", "cov_kf", "cov_weight")} == cov
    assert a1["keyframe"].mOrderedCovGraph == [(40, 0)]
    # CreateInitialMapRGBD's test of :182: too few points, nothing written
    empty = track_map.TrackMapStore(mctx)
    f2 = Frame(cam, pyr, T0.reshape(3, 4))
    assert trk.CreateInitialMapRGBD(empty, np.zeros_like(depth), f2) is None and f2.n_features == 0 and len(empty.points) == len(empty.keyframes) == 0
    r = empty.map.read()
    assert len(r["p_world"]) == 0 and len(r["slots"]) == 0


def test_multitracker_craete_keyframes_equals_the_single_calls():
    """MultiTracker.CraeteKeyframes for three sequences (own stores) in one dsdtm_newkf_make_batch: each store's map equals the one
    Tracker.CraeteKeyframe builds for that sequence alone."""
    from dsdtm_amd import track_map, tracking
    from dsdtm_amd.frame import Frame
    gpu = capi.default_context(0)
    w, h = 640, 480
    cam = synth.Camera.tum(w, h)
    rng = np.random.default_rng(33)
    tctx = track_map.TrackMapContext(0)
    frames = lambda: [Frame(cam, synth.build_pyramid(np.clip(np.rint(synth.make_texture(h, w, 40 + i)), 0, 255).astype(np.uint8), 5), T[i].reshape(3, 4))
                      for i in range(3)]
    T = [cases.pose(rng) for _ in range(3)]
    depths = [cases.random_depth(rng, R.NewKeyframeParams(w, h, 1, 1, 1, 1, 1), zeros=0.2) for _ in range(3)]
    multi, single = tracking.MultiTracker(cam, gpu), tracking.Tracker(cam, gpu)
    sa, sb = [track_map.TrackMapStore(tctx) for _ in range(3)], [track_map.TrackMapStore(tctx) for _ in range(3)]
    fa, fb = frames(), frames()
    outs = multi.CraeteKeyframes(fa, sa, depths)
    for i in range(3):
        one = single.CraeteKeyframe(sb[i], depths[i], cur=fb[i])
        assert outs[i]["n_new"] == one["n_new"] > 20 and outs[i]["cov"] is None and np.array_equal(fa[i].px, fb[i].px)
        ga, gb = sa[i].map.read(), sb[i].map.read()
        assert ga["p_world"].tobytes() == gb["p_world"].tobytes() and len(ga["p_world"]) > 20
        assert all(np.array_equal(ga[k][0], gb[k][0]) for k in ("slots", "observes", "px", "level", "bearing"))
