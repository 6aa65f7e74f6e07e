"""dsdtm_track_frames on RESIDENT frames (descs[f].image == NULL, results[f].frame names frame f): the batch entry starting at Run on
frames that are already on the device or on their way there — pending prefetches (with and without a depth map), frames of
dsdtm_frame_create_from_image, members of an older batch's slab. Held to the image batch byte for byte, to dsdtm_track_frame_on
frame by frame, and through MultiTracker.prefetch / TrackFrames to the same sequences tracked alone."""
import copy
import ctypes as C

import numpy as np
import pytest

from dsdtm_amd import capi, synth, tracking, tum
from dsdtm_amd.frame import Config
from tests import rgbd_restatement as R
from tests.test_frame_prefetch_gpu import depth_map, lift_all, pyramid_levels, same_pyramid
from tests.test_search_gpu import make_world
from tests.test_track_frames_gpu import ALIGN, _as_ref, _in_grid_by_host, _last_with, _same, _sequence_world, _set_config

pytestmark = pytest.mark.gpu

LEVELS = 5


def _frame(world, nf, **kw):
    cam, kfs, cur, mps = world
    f = dict(image=np.ascontiguousarray(cur.mvImg_Pyr[0]), levels=LEVELS, last=_last_with(kfs[0], cam, nf), T_seed=kfs[0].Get_Pose(),
             align=ALIGN, min_tracked=20, keyframes=kfs, map_points=mps)
    f.update(kw)
    return f


def _raw(call):
    """Every byte the call wrote: each result behind its `frame` member, the whole match, residual-norm and in-grid arrays."""
    off = capi.TrackResult.T_run.offset
    return ([bytes(call.res[f])[off:] for f in range(call.n)], call.matches.tobytes(), call.rn.tobytes(), call.in_grid.tobytes())


def _on(ctx, cam, f, df):
    """dsdtm_track_frame_on on frame `df` with the descriptor of `f`."""
    kw = {k: v for k, v in f.items() if k not in ("image", "levels", "last", "T_seed", "align", "min_tracked", "keyframes", "map_points")}
    return tracking.track_frame(ctx, cam, None, f["levels"], f["last"], f["T_seed"], f["align"], f["min_tracked"], f["keyframes"],
                                f["map_points"], cur_frame=df, **kw)


@pytest.fixture(scope="module")
def worlds():
    _set_config()
    return [make_world(s, n_points=n) for s, n in ((111, 700), (112, 600))]


@pytest.fixture(scope="module")
def odd_worlds():
    """636 x 478: level widths 636, 318, 159, 80, 40 — no multiple of 16 below level 3, level offsets unlike 640 x 480's."""
    _set_config()
    return [make_world(s, n_points=500, n_kf=2, width=636, height=478) for s in (121, 122)]


def test_heterogeneous_batch_on_pending_frames_equals_the_image_batch(gpu_ctx, worlds):
    """Six frames, reference feature counts in the bands of 128, 320 and 704, among them a frame Run loses (a seed pose from which no
    feature is in the image), one with an empty local map and one below Min_fts; a mask on one. Every frame is prefetched and not
    waited for. results (behind `frame`), matches, residual norms and in-grid flags equal the call on the images in every byte; the
    frames are the ones that went in, their pyramids those of the image batch."""
    _set_config()
    cam = worlds[0][0]
    far = np.array(worlds[0][1][0].Get_Pose(), np.float64).copy()
    far[0, 3] += 100.0
    mask = np.full((cam.height, cam.width), 255, np.uint8); mask[150:260, :] = 0
    frames = [_frame(worlds[0], 100), _frame(worlds[1], 300, mask=mask), _frame(worlds[0], 600), _frame(worlds[1], 200, T_seed=far),
              _frame(worlds[0], 280, map_points=[]), _frame(worlds[1], 10)]
    a = tracking.TrackBatchCall(gpu_ctx, cam, frames)
    ra = a.run()
    dfs = [capi.DeviceFrame.prefetch(gpu_ctx, f["image"].copy(), LEVELS) for f in frames]      # pending when the call starts
    b = tracking.TrackBatchCall(gpu_ctx, cam, frames, cur_frames=dfs)
    assert b.resident and all(d.image is None for d in b.descs)
    rb = b.run()
    assert [b.res[f].frame for f in range(6)] == [df.handle.value for df in dfs] and all(r["frame"] is df for r, df in zip(rb, dfs))
    wa, wb = _raw(a), _raw(b)
    for f in range(6):
        assert wa[0][f] == wb[0][f], f"frame {f}: result"
    assert wa[1] == wb[1] and wa[2] == wb[2] and wa[3] == wb[3]
    assert ra[3]["lost"] and ra[3]["n_tracked"] < 20                                            # Run ran (200 features) and lost it
    assert ra[5]["lost"] and ra[5]["n_tracked"] == 0 and np.array_equal(ra[5]["T_run"], frames[5]["T_seed"])
    assert ra[4]["n_in_grid"] == 0 and not ra[4]["lost"]
    assert sum(len(r["matches"]) > 30 for r in ra) >= 3
    for f in range(6):
        assert same_pyramid(pyramid_levels(dfs[f], cam.width, cam.height), pyramid_levels(ra[f]["frame"], cam.width, cam.height)), f
    # the same frames, settled now, give the same again
    b.run()
    assert _raw(b) == wb
    for r, df in zip(ra, dfs):
        r["frame"].close(); df.close()


@pytest.mark.parametrize("size", ["640x480", "636x478"])
def test_frames_of_mixed_origins_in_any_order_equal_track_frame_on(gpu_ctx, worlds, odd_worlds, size):
    """The pointer table is what addresses the frames: a pending prefetch with a depth map, a frame of create_from_image and two
    members of an older batch's slab, handed in in an order that is neither allocation order nor band order (the call sorts by
    band: 300, 100, 400, 200 features -> slots 2, 0, 3, 1), then reversed. Each frame's results are its dsdtm_track_frame_on's."""
    _set_config()
    ws = worlds if size == "640x480" else odd_worlds
    cam = ws[0][0]
    imgs = [np.ascontiguousarray(ws[j % 2][2].mvImg_Pyr[0]) for j in range(4)]
    imgs[2] = np.ascontiguousarray(imgs[2][::-1])                      # (four different images: a frame read through another's entry shows)
    imgs[3] = np.ascontiguousarray(imgs[3][:, ::-1])
    old = tracking.track_frames(gpu_ctx, cam, [_frame(ws[0], 100, image=imgs[0]), _frame(ws[1], 100, image=imgs[1])])
    d16 = depth_map(cam.width, cam.height, 5)
    dfs = [old[1]["frame"], capi.DeviceFrame.prefetch(gpu_ctx, imgs[2].copy(), LEVELS, depth=d16, depth_scale=5000.0), old[0]["frame"],
           capi.DeviceFrame.from_image(gpu_ctx, imgs[3], LEVELS)]
    descs = [_frame(ws[1], 300, image=None), _frame(ws[0], 100, image=None), _frame(ws[0], 400, image=None), _frame(ws[1], 200, image=None)]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0]):
        got = tracking.track_frames(gpu_ctx, cam, [descs[i] for i in order], cur_frames=[dfs[i] for i in order])
        for g, i in zip(got, order):
            assert g["frame"] is dfs[i]
            want = _on(gpu_ctx, cam, descs[i], dfs[i])
            _same(g, want, f"{size}, order {order}, frame {i}")
            if not g["lost"]:
                assert np.array_equal(g["in_grid"], _in_grid_by_host(cam, g["T_run"], descs[i]["map_points"])), i
    assert sum(len(g["matches"]) > 20 for g in got) >= 2
    # the depth map came through both calls
    px = np.stack(np.meshgrid(np.arange(0, cam.width, 7), np.arange(0, cam.height, 5)), -1).reshape(-1, 2).astype(np.float32)
    got_d, _ = lift_all(dfs[1], cam, np.eye(4)[:3], px)
    plane = tum.depth_to_metres(d16, 5000.0)
    at = d16[px[:, 1].astype(int), px[:, 0].astype(int)] != 0
    assert np.array_equal(got_d[at].view(np.uint32), plane[px[at, 1].astype(int), px[at, 0].astype(int)].view(np.uint32))
    for df in dfs:
        df.close()


def test_one_resident_frame_equals_track_frame_on(gpu_ctx, odd_worlds):
    _set_config()
    cam = odd_worlds[0][0]
    f = _frame(odd_worlds[0], 250)
    df = capi.DeviceFrame.prefetch(gpu_ctx, f["image"].copy(), LEVELS)
    got = tracking.track_frames(gpu_ctx, cam, [dict(f, image=None)], cur_frames=[df])
    want = _on(gpu_ctx, cam, f, df)
    _same(got[0], want, "n = 1")
    assert got[0]["frame"] is df and len(got[0]["matches"]) > 30
    df.close()


def test_lockstep_rgbd_sequences_equal_the_same_sequences_tracked_alone(gpu_ctx, gpu_ctx_diag):
    """Two trackers, four steps through MultiTracker.prefetch / TrackFrames, step k + 1 prefetched (gray + depth) BEFORE step k is
    tracked, against each sequence alone through Tracker.TrackFrame (diagnostic library, teams off: the first reference frames
    have 449..704 features, which the batch runs on one compute unit). Poses, matches, refined pixels, found counts, bad flags and
    the projected local map points agree at every step; on the last step each tracked frame's depth plane is
    tum.depth_to_metres' bit for bit and its lift the restatement's within the bound of tests/test_frame_prefetch_gpu.py."""
    _set_config()
    n_seq, n_kf, steps = 2, 2, 4
    worlds = [_sequence_world(340 + s, n_kf) for s in range(n_seq)]
    cam = worlds[0][0]
    depths = [[depth_map(cam.width, cam.height, 50 + 10 * s + k) for k in range(steps)] for s in range(n_seq)]
    alone = []
    with capi.debug_options(no_team=1):
        for cam_s, kfs, mps, imgs in copy.deepcopy(worlds):
            trk = tracking.Tracker(cam_s, ctx=gpu_ctx_diag, max_level=5, min_level=0, max_iters=8, min_tracked=20)
            idx = {id(mp): i for i, mp in enumerate(mps)}
            log, last = [], kfs[n_kf - 1]
            for k in range(steps):
                bad0 = [mp.IsBad() for mp in mps]
                cur, n, matches = trk.TrackFrame(imgs[k], last, kfs, mps)
                r = trk.last_result
                log.append(dict(n=n, T_run=r["T_run"].copy(), T_opt=cur.Get_Pose().copy(), matches=[(m[0], idx[id(m[1])], m[3]) for m in matches],
                                px=np.array([m[2] for m in matches]), found=[mp.mnFound for mp in mps], bad=[mp.mbBad for mp in mps],
                                n_in_grid=r["n_in_grid"], in_grid=_in_grid_by_host(cam_s, r["T_run"], mps, bad0) if not r["lost"] else np.zeros(len(mps), np.uint8)))
                last = cur
            alone.append(log)
    b = copy.deepcopy(worlds)
    mt = tracking.MultiTracker(cam, ctx=gpu_ctx, max_level=5, min_level=0, max_iters=8, min_tracked=20)
    lasts = [w[1][n_kf - 1] for w in b]
    sent = {0: mt.prefetch([w[3][0] for w in b], [depths[s][0] for s in range(n_seq)])}
    prev = None
    for k in range(steps):
        if k + 1 < steps:
            sent[k + 1] = mt.prefetch([w[3][k + 1] for w in b], [depths[s][k + 1] for s in range(n_seq)])
        out = mt.TrackFrames([w[3][k] for w in b], lasts, [w[1] for w in b], [w[2] for w in b])
        for s, (cur, n, matches) in enumerate(out):
            a, r = alone[s][k], mt.last_results[s]
            assert r["frame"] is sent[k][s] and cur._device_frame is sent[k][s], (s, k)
            idx = {id(mp): i for i, mp in enumerate(b[s][2])}
            assert n == a["n"] and np.array_equal(r["T_run"], a["T_run"]), (s, k)
            assert [(m[0], idx[id(m[1])], m[3]) for m in matches] == a["matches"], (s, k)
            assert np.array_equal(np.array([m[2] for m in matches]), a["px"]), (s, k)
            assert np.array_equal(cur.Get_Pose(), a["T_opt"]), (s, k)
            assert [mp.mnFound for mp in b[s][2]] == a["found"] and [mp.mbBad for mp in b[s][2]] == a["bad"], (s, k)
            assert r["n_in_grid"] == a["n_in_grid"] and np.array_equal(r["in_grid"], a["in_grid"]), (s, k)
            assert [id(mp) for mp in r["local_map_points"]] == [id(b[s][2][i]) for i in np.flatnonzero(a["in_grid"])]
        if prev is not None:
            for fr in prev:
                fr._device_frame.close()
        prev = [o[0] for o in out]
        lasts = prev
    assert not mt._prefetched and all(alone[s][-1]["n"] >= 40 for s in range(n_seq))
    # the keyframe decision of the last step: the lift on each tracker's resident frame
    yy, xx = np.mgrid[0:cam.height, 0:cam.width]
    every = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float32)
    rng = np.random.default_rng(4)
    for s in range(n_seq):
        df, T = mt.last_results[s]["frame"], np.asarray(lasts[s].Get_Pose(), np.float64)
        d16 = depths[s][steps - 1]
        plane = tum.depth_to_metres(d16, 5000.0)
        got, _ = lift_all(df, cam, T, every)
        got = got.reshape(cam.height, cam.width)
        assert np.array_equal(got[d16 != 0].view(np.uint32), plane[d16 != 0].view(np.uint32))
        px = rng.uniform(0, [cam.width - 1, cam.height - 1], (400, 2)).astype(np.float32)
        got_d, got_p = df.lift(cam, T, px)
        want_d, want_p = R.lift(plane, cam, T, px)
        assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32)) and (got_d != -1).sum() >= 300
        worst = 0.0
        for i in range(len(px)):
            if want_d[i] == -1:
                assert np.all(got_p[i] == 0)
                continue
            d = float(want_d[i])
            p_c = max(abs(d * (float(px[i, 0]) - cam.cx) / cam.fx), abs(d * (float(px[i, 1]) - cam.cy) / cam.fy), d)
            worst = max(worst, float(np.abs(got_p[i] - want_p[i]).max()) / R.ulp_bound(p_c, float(np.abs(T[:, 3]).max())))
        print(f"tracker {s}: lift, largest difference / (4 ulp bound) {worst:.3f}")
        assert worst <= 1.0
    for fr in prev:
        fr._device_frame.close()


def test_destruction_and_frames_of_a_call_as_ref_and_kf_of_the_next(worlds):
    """A context of its own, destroyed last. One frame of a call is destroyed while the others live; a frame of the call is the
    reference frame, another a keyframe, of the next call — issued at once, on frames that are pending again."""
    _set_config()
    ctx = capi.Context(0)
    cam, kfs, cur, mps = worlds[0]
    f = [_frame(worlds[0], nf, image=None) for nf in (150, 300, 90)]
    img = np.ascontiguousarray(cur.mvImg_Pyr[0])
    dfs = [capi.DeviceFrame.prefetch(ctx, img.copy(), LEVELS) for _ in range(3)]
    got = tracking.track_frames(ctx, cam, f, cur_frames=dfs)
    want = [_on(ctx, cam, f[i], dfs[i]) for i in range(3)]
    for i in range(3):
        _same(got[i], want[i], f"first call, frame {i}")
    dfs[1].close()
    nxt = [capi.DeviceFrame.prefetch(ctx, np.ascontiguousarray(worlds[0][1][1].mvImg_Pyr[0]).copy(), LEVELS) for _ in range(2)]
    kf2 = copy.copy(kfs[1]); kf2._device_frame = dfs[2]
    g = [dict(f[0], last=_as_ref(f[0]["last"], dfs[0]), keyframes=[kfs[0], kf2] + list(kfs[2:])), dict(f[2], last=_as_ref(f[2]["last"], dfs[0]))]
    got2 = tracking.track_frames(ctx, cam, g, cur_frames=nxt)
    for i in range(2):
        _same(got2[i], _on(ctx, cam, g[i], nxt[i]), f"second call, frame {i}")
    assert got2[0]["n_tracked"] > 20
    nxt[0].close(); dfs[2].close(); dfs[0].close(); nxt[1].close()
    for k in kfs:
        df = getattr(k, "_device_frame", None)
        if df is not None and df.ctx is ctx:
            df.close(); k._device_frame = None
    for fr in f:
        df = getattr(fr["last"], "_device_frame", None)
        if df is not None and df.ctx is ctx:
            df.close()
    ctx.close()


def test_argument_errors_name_frame_and_field_and_leave_the_frames_usable(gpu_ctx, worlds):
    _set_config()
    cam = worlds[0][0]
    f = [_frame(worlds[0], 120, image=None), _frame(worlds[1], 200, image=None), _frame(worlds[0], 300, image=None)]
    dfs = [capi.DeviceFrame.prefetch(gpu_ctx, np.ascontiguousarray(worlds[j % 2][2].mvImg_Pyr[0]).copy(), LEVELS) for j in range(3)]
    before = [_on(gpu_ctx, cam, f[i], dfs[i]) for i in range(3)]
    call = tracking.TrackBatchCall(gpu_ctx, cam, f, cur_frames=dfs)
    lib = gpu_ctx.lib
    handles = [df.handle.value for df in dfs]
    img = np.ascontiguousarray(worlds[0][2].mvImg_Pyr[0])

    def refused(frame, field, frames=handles):
        for i in range(3):
            call.res[i].frame = frames[i]
        rc = lib.dsdtm_track_frames(gpu_ctx.handle, C.byref(call.cs), 3, call.descs, call.res, call.matches.ctypes.data, call.rn.ctypes.data,
                                    call.in_grid.ctypes.data)
        msg = lib.dsdtm_last_error(gpu_ctx.handle).decode()
        assert rc == capi.ERR_INVALID and f"frame {frame}" in msg and field in msg, (rc, msg)
        assert [call.res[i].frame for i in range(3)] == list(frames), msg          # the caller's, untouched

    call.descs[1].image = img.ctypes.data                                         # a mixture
    refused(1, "image")
    call.descs[1].image = None
    refused(2, "results[2].frame is NULL", handles[:2] + [None])
    refused(2, "also frame 0", [handles[0], handles[1], handles[0]])             # the same frame twice
    keep = call.descs[1].ref
    call.descs[1].ref = handles[1]                                                # its own reference frame
    refused(1, "ref")
    call.descs[1].ref = keep
    for field, value in (("width", cam.width - 4), ("height", cam.height - 2), ("levels", LEVELS - 1)):
        old = getattr(call.descs[0], field)
        for d in call.descs:
            setattr(d, field, value)
        refused(0, field)
        for d in call.descs:
            setattr(d, field, old)
    if lib.dsdtm_device_count() > 1:
        other = capi.Context(1)
        foreign = capi.DeviceFrame.from_image(other, img, LEVELS)
        refused(1, "another context", [handles[0], foreign.handle.value, handles[2]])
        foreign.close(); other.close()
    # nothing was enqueued and nothing taken: every frame tracks as before, alone and in the call
    for i in range(3):
        _same(_on(gpu_ctx, cam, f[i], dfs[i]), before[i], f"frame {i} afterwards")
    got = call.run()
    for i in range(3):
        _same(got[i], before[i], f"frame {i} in the call")
    for df in dfs:
        df.close()
