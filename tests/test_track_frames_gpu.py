"""dsdtm_track_frames — the frames of n independent trackers tracked in ONE call. Every frame must be what dsdtm_track_frame makes
of the same descriptor, bit for bit (Run, search, replay, refinement, the returned pyramid), whatever else shares the batch; the
per-point in-grid flags must be ReprojectPoint's answers; sequences tracked in lockstep must equal the same sequences tracked
alone; and the call is all or nothing."""
import copy
import ctypes as C
import threading

import numpy as np
import pytest

from dsdtm_amd import capi, search, synth, tracking
from dsdtm_amd.frame import Config, Frame
from tests import helpers as H
from tests import quirk_fixtures as Q
from tests.test_search_gpu import make_world

pytestmark = pytest.mark.gpu

ALIGN = (5, 0, 8, 15)


def _set_config(cell=25):
    Config.Set("Camera.CellSize", cell); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)


def _last_with(ref, cam, nf):
    nf = min(nf, ref.n_features)
    bb = ref.bearing[:nf]
    last = Frame(cam, ref.mvImg_Pyr, ref.Get_Pose())
    last.set_features(ref.px[:nf], bb, bb * (2.0 / bb[:, 2:3]), np.ones(nf, np.uint8))
    return last


def _same(a, b, what=""):
    assert np.array_equal(a["T_run"], b["T_run"]), what + ": T_run"
    assert a["n_tracked"] == b["n_tracked"] and a["lost"] == b["lost"], what
    for k in a["stats"]:
        assert np.array_equal(np.asarray(a["stats"][k]), np.asarray(b["stats"][k])), (what, k)
    assert a["n_in_grid"] == b["n_in_grid"] and a["replay_full_scan"] == b["replay_full_scan"], what
    assert np.array_equal(a["matches"], b["matches"]), what + ": matches"
    assert np.array_equal(a["T_opt"], b["T_opt"]), what + ": T_opt"
    for k in ("iterations", "successful_steps", "termination", "n_residual_blocks", "initial_cost", "final_cost"):
        assert a["summary"][k] == b["summary"][k], (what, k)
    assert np.array_equal(a["summary"]["x"], b["summary"]["x"]), what
    assert np.array_equal(a["residual_norm"], b["residual_norm"]), what


def _as_ref(last, df):
    """`last` (pose, features) over another device pyramid: a frame of a batch or of a single call."""
    fr = copy.copy(last)
    fr._device_frame = df
    return fr


def _single(ctx, cam, f):
    kw = {k: v for k, v in f.items() if k not in ("image", "levels", "last", "T_seed", "align", "min_tracked", "keyframes", "map_points")}
    return tracking.track_frame(ctx, cam, f["image"], f["levels"], f["last"], f["T_seed"], f["align"], f["min_tracked"],
                                f["keyframes"], f["map_points"], **kw)


def _in_grid_by_host(cam, T, mps, bad=None):
    """LocalPointSearch.ReprojectPoint's answer per point with the pose Run produced; bad points (`bad`: as they were when the
    frame was tracked) are not projected."""
    s = search.LocalPointSearch(cam, resident_frames=False)
    s.ResetGrid()
    cur = Frame(cam, [np.zeros((cam.height, cam.width), np.uint8)], T)
    bad = [mp.IsBad() for mp in mps] if bad is None else bad
    return np.array([0 if b else int(s.ReprojectPoint(cur, mp)) for mp, b in zip(mps, bad)], np.uint8)


def test_heterogeneous_batch_equals_the_single_call_frame_by_frame(gpu_ctx):
    """About a dozen frames that share only the camera and the tracking parameters: reference feature counts over five register
    bands, an empty local map, no keyframes, a lost frame (too few features for Run), a mask that blocks everything, a half mask.
    Each frame equals dsdtm_track_frame on its descriptor in every field; its pyramid, as the reference frame of a next call,
    gives what the single call's pyramid gives; its in-grid flags are ReprojectPoint's."""
    _set_config()
    worlds = [make_world(s, n_points=n) for s, n in ((101, 700), (102, 900), (103, 500))]
    frames = []
    for j, nf in enumerate((100, 150, 250, 300, 400, 180, 120, 200, 260, 10, 220, 330)):
        cam, kfs, cur, mps = worlds[j % 3]
        last = _last_with(kfs[0], cam, nf)
        f = dict(image=cur.mvImg_Pyr[0], levels=5, last=last, T_seed=kfs[0].Get_Pose(), align=ALIGN, min_tracked=20,
                 keyframes=kfs, map_points=mps)
        if j == 5:
            f["map_points"] = []                                          # an empty local map
        if j == 6:
            f["keyframes"], f["map_points"] = [], []                      # no keyframes at all
        if j == 7:
            f["mask"] = np.zeros((cam.height, cam.width), np.uint8)       # blocks everything
        if j == 8:
            m = np.full((cam.height, cam.width), 255, np.uint8); m[150:260, :] = 0
            f["mask"] = m
        frames.append(f)
    cam = worlds[0][0]
    got = tracking.track_frames(gpu_ctx, cam, frames)
    assert len(got) == len(frames)
    bands = set()
    for j, (f, g) in enumerate(zip(frames, got)):
        want = _single(gpu_ctx, cam, f)
        _same(g, want, f"frame {j}")
        if j < 4:
            # the returned pyramids: as reference frames of a next single call, the batch's and the single call's give the same bits
            nxt = dict(f, image=worlds[(j + 1) % 3][2].mvImg_Pyr[0], T_seed=g["T_opt"])
            r_b = _single(gpu_ctx, cam, dict(nxt, last=_as_ref(f["last"], g["frame"])))
            r_s = _single(gpu_ctx, cam, dict(nxt, last=_as_ref(f["last"], want["frame"])))
            _same(r_b, r_s, f"frame {j}: pyramid")
            r_b["frame"].close(); r_s["frame"].close()
        assert int(g["in_grid"].sum()) == g["n_in_grid"] and len(g["in_grid"]) == len(f["map_points"])
        if g["lost"]:
            assert not g["in_grid"].any()
        else:
            assert np.array_equal(g["in_grid"], _in_grid_by_host(cam, g["T_run"], f["map_points"])), f"frame {j}: in-grid flags"
        bands.add(capi_band(f["last"].n_features))
        want["frame"].close()
    assert got[9]["lost"] and got[9]["n_tracked"] == 0 and np.array_equal(got[9]["T_run"], frames[9]["T_seed"])
    assert got[5]["n_in_grid"] == 0 and got[6]["n_in_grid"] == 0 and len(got[7]["matches"]) == 0 and got[7]["n_in_grid"] > 100
    assert sum(len(g["matches"]) > 30 for g in got) >= 6
    assert len(bands) >= 5
    # destroyed in shuffled order
    for j in np.random.default_rng(5).permutation(len(got)):
        got[j]["frame"].close()


def capi_band(nf):
    return next(i for i, hi in enumerate((128, 192, 256, 320, 448, 704)) if nf <= hi)


@pytest.mark.parametrize("width,height", [(640, 480), (636, 478)])
def test_every_way_an_image_can_arrive_in_a_batch(gpu_ctx, width, height):
    """One image-mode call whose six frames' images arrive on every route of dsdtm_track_frames, in this order: device memory
    row-strided (the copy engine — this frame has the fewest features, so it stays in slot 0 behind the sort by register band and
    Run's range gets an ingest launch of its own), pageable, pageable row-strided (both staged), pinned and aligned (read in place),
    pinned at address + 4 (the copy engine), device memory aligned (read in place). Then a call of two frames, both at odd device
    addresses. Every frame equals dsdtm_track_frame on the same pageable image, and its pyramid is DeviceFrame.from_image's.
    636 x 478: the byte count is no multiple of 16, the level widths are 636/318/159/80/40."""
    import torch
    from tests.test_frame_prefetch_gpu import pyramid_levels, same_pyramid
    _set_config()
    cam, kfs, cur, mps = make_world(31, n_points=500, n_kf=2, width=width, height=height)
    n = width * height
    rng = np.random.default_rng(9)
    images = [np.ascontiguousarray(cur.mvImg_Pyr[0])]
    for _ in range(5):                                                 # the same scene under a little noise: six different images
        images.append(np.clip(images[0].astype(np.int16) + rng.integers(-2, 3, images[0].shape), 0, 255).astype(np.uint8))
    frames = [dict(image=im, levels=5, last=_last_with(kfs[0], cam, nf), T_seed=kfs[0].Get_Pose(), align=ALIGN, min_tracked=20,
                   keyframes=kfs, map_points=mps) for im, nf in zip(images, (100, 150, 250, 300, 180, 120))]
    assert capi_band(frames[0]["last"].n_features) == 0 and frames[0]["last"].n_features < min(f["last"].n_features for f in frames[1:])
    want = [_single(gpu_ctx, cam, f) for f in frames]
    pyr = []
    for im in images:
        df = capi.DeviceFrame.from_image(gpu_ctx, im, 5)
        pyr.append(pyramid_levels(df, width, height, 5))
        df.close()

    keep = []
    def device(im, stride, at=0):
        t = torch.zeros(height * stride + 64, dtype=torch.uint8, device="cuda")
        t[at:at + height * stride].reshape(height, stride)[:, :width] = torch.from_numpy(im).cuda()
        keep.append(t)
        assert t.data_ptr() % 16 == 0
        return t.data_ptr() + at, stride

    def pinned(im, at=0):
        t = torch.empty(n + 64, dtype=torch.uint8).pin_memory()
        a = t.numpy()[at:at + n].reshape(height, width)
        a[:] = im
        keep.append(t)
        assert a.ctypes.data % 16 == at
        return a.ctypes.data, width

    def check(call, idx, arrivals):
        for j, (ptr, stride) in enumerate(arrivals):
            if ptr is not None:
                call.descs[j].image, call.descs[j].stride = ptr, stride
        torch.cuda.synchronize()
        got = call.run()
        for j, g in zip(idx, got):
            _same(g, want[j], f"frame {j}")
            assert same_pyramid(pyramid_levels(g["frame"], width, height, 5), pyr[j]), f"frame {j}: pyramid"
            g["frame"].close()
        return got

    strided = np.zeros((height, width + 7), np.uint8)[:, :width]; strided[:] = images[2]
    six = [dict(f) for f in frames]
    six[2]["image"] = strided
    got = check(tracking.TrackBatchCall(gpu_ctx, cam, six), range(6),
                [device(images[0], width + 40), (None, None), (None, None), pinned(images[3]), pinned(images[4], 4), device(images[5], width)])
    assert sum((not g["lost"]) and len(g["matches"]) > 20 for g in got) >= 3
    check(tracking.TrackBatchCall(gpu_ctx, cam, [dict(frames[1]), dict(frames[4])]), (1, 4), [device(images[1], width, 4), device(images[4], width, 4)])
    for w in want:
        w["frame"].close()


@pytest.mark.parametrize("name", list(Q.SEARCH_WORLDS))
def test_search_worlds_in_a_batch_equal_the_restatement(gpu_ctx, name):
    """The quirk worlds (tests/quirk_fixtures.py) as frames of a batch of three: each equals the single call, the sequential
    restatement of the search and the committed arrays of tests/golden/quirks.npz."""
    cam, kfs, cur, mps, cell = Q.search_world(name)
    last = Frame(cam, cur.mvImg_Pyr, cur.Get_Pose())
    mask0 = Q.search_mask(name)
    f = dict(image=cur.mvImg_Pyr[0], levels=5, last=last, T_seed=cur.Get_Pose(), align=ALIGN, min_tracked=0, keyframes=kfs,
             map_points=mps, cell_size=cell, max_pyr_levels=5, mask=mask0.copy())
    got = tracking.track_frames(gpu_ctx, cam, [dict(f), dict(f, mask=mask0.copy()), dict(f, mask=mask0.copy())])
    want = _single(gpu_ctx, cam, dict(f, mask=mask0.copy()))
    g = np.load(H.golden_path("quirks.npz"))
    restated = Q.search_restated(name)
    for r in got:
        _same(r, want, name)
        m = r["matches"]
        lst = [(int(m["cell"][k]), int(m["point"][k]), float(m["px"][k][0]), float(m["px"][k][1]), int(m["level"][k])) for k in range(len(m))]
        mask = mask0.copy()
        for q in m["px"]:
            search.fill_circle(mask, search.cvRound(float(q[0])), search.cvRound(float(q[1])), cell, 0)
        assert Q.search_first_difference(restated, (lst, mask, int(r["n_in_grid"]))) is None
        assert np.array_equal(np.array(lst, np.float64).reshape(-1, 5), g[f"search_{name}_matches"])
        assert int(r["n_in_grid"]) == int(g[f"search_{name}_n_in_grid"]) == int(r["in_grid"].sum())
        r["frame"].close()
    want["frame"].close()


def test_replay_full_scan_in_a_batch(gpu_ctx):
    """4096 map points over cells of 40 px (the replay's full scan) beside a small frame: both equal their single calls."""
    _set_config(40)
    try:
        cam, kfs, cur, mps = make_world(13, n_points=4096, cell=40, obs_margin=3)
        cam2, kfs2, cur2, mps2 = make_world(14, n_points=300, cell=40)
        last = Frame(cam, cur.mvImg_Pyr, cur.Get_Pose())
        last2 = _last_with(kfs2[0], cam2, 200)
        fs = [dict(image=cur.mvImg_Pyr[0], levels=5, last=last, T_seed=cur.Get_Pose(), align=ALIGN, min_tracked=0, keyframes=kfs,
                   map_points=mps, cell_size=40),
              dict(image=cur2.mvImg_Pyr[0], levels=5, last=last2, T_seed=kfs2[0].Get_Pose(), align=ALIGN, min_tracked=0, keyframes=kfs2,
                   map_points=mps2, cell_size=40)]
        got = tracking.track_frames(gpu_ctx, cam, fs)
        assert got[0]["replay_full_scan"] and len(got[0]["matches"]) >= 100
        for j, (f, g) in enumerate(zip(fs, got)):
            want = _single(gpu_ctx, cam, f)
            _same(g, want, f"frame {j}")
            want["frame"].close(); g["frame"].close()
    finally:
        Config.Set("Camera.CellSize", 25)


def _sequence_world(seed, n_kf=2):
    cam, kfs, _, mps = make_world(seed, n_points=700, n_kf=n_kf)
    for k, kf in enumerate(kfs):
        mpts = [None] * kf.n_features
        for mp in mps:
            if k in mp.mObservations:
                mpts[mp.mObservations[k]] = mp
        kf.mvMapPoints = mpts
        kf.p_world = np.array([m_.mPose if m_ is not None else np.zeros(3) for m_ in mpts])
        kf.initial = np.array([1 if m_ is not None else 0 for m_ in mpts], np.uint8)
    rng = np.random.default_rng(seed + 1000)
    tex = synth.make_texture(cam.height, cam.width, seed)
    T0 = np.vstack([kfs[n_kf - 1].Get_Pose(), [0, 0, 0, 1]])
    imgs, xi = [], np.zeros(6)
    for _ in range(7):
        xi = xi + np.concatenate([rng.uniform(-0.012, 0.012, 3), rng.uniform(-0.006, 0.006, 3)])
        imgs.append(synth.warp_plane(tex, cam, synth.se3_exp(xi) @ T0, 2.0))
    return cam, kfs, mps, imgs


def test_lockstep_sequences_equal_the_same_sequences_tracked_alone(gpu_ctx, gpu_ctx_diag):
    """Eight independent sequences of seven frames: one dsdtm_track_frames per step (MultiTracker; batch k's frames are the reference
    frames of batch k + 1 and are destroyed in shuffled order) against each sequence alone through Tracker.TrackFrame. Poses, counts,
    matches, refined pixels, map side effects (found counts, bad flags) and the projected local map points agree, frame after frame.
    (The first reference frames are keyframes of 449..704 features, whose single-call Run is a team of compute units; the batch runs
    them on one: the sequences alone run on the diagnostic library with teams switched off.)"""
    _set_config()
    n_seq, n_kf = 8, 2
    worlds = [_sequence_world(300 + s, n_kf) for s in range(n_seq)]
    cam = worlds[0][0]
    alone = []
    with capi.debug_options(no_team=1):
        for cam_s, kfs, mps, imgs in copy.deepcopy(worlds):
            trk = tracking.Tracker(cam_s, ctx=gpu_ctx_diag, max_level=5, min_level=0, max_iters=8, min_tracked=20)
            idx = {id(mp): i for i, mp in enumerate(mps)}
            log, last = [], kfs[n_kf - 1]
            for k in range(7):
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
    prev = None
    rng = np.random.default_rng(9)
    for k in range(7):
        out = mt.TrackFrames([w[3][k] for w in b], lasts, [w[1] for w in b], [w[2] for w in b])
        for s, (cur, n, matches) in enumerate(out):
            a, r = alone[s][k], mt.last_results[s]
            idx = {id(mp): i for i, mp in enumerate(b[s][2])}
            assert n == a["n"] and np.array_equal(r["T_run"], a["T_run"]), (s, k)
            assert [(m[0], idx[id(m[1])], m[3]) for m in matches] == a["matches"], (s, k)
            assert np.array_equal(np.array([m[2] for m in matches]), a["px"]), (s, k)
            assert np.array_equal(cur.Get_Pose(), a["T_opt"]), (s, k)
            assert [mp.mnFound for mp in b[s][2]] == a["found"] and [mp.mbBad for mp in b[s][2]] == a["bad"], (s, k)
            assert r["n_in_grid"] == a["n_in_grid"] and np.array_equal(r["in_grid"], a["in_grid"]), (s, k)
            assert [id(mp) for mp in r["local_map_points"]] == [id(b[s][2][i]) for i in np.flatnonzero(a["in_grid"])]
        if prev is not None:                                           # the previous batch's frames: no longer referenced
            for j in rng.permutation(len(prev)):
                prev[j]._device_frame.close()
        prev = [o[0] for o in out]
        lasts = prev
    assert all(alone[s][-1]["n"] >= 40 for s in range(n_seq))


def test_run_of_600_features_in_a_batch(gpu_ctx, gpu_ctx_diag):
    """600 reference features: the batch runs them on one compute unit — bit for bit what the single call gives with teams switched
    off (diagnostic library), and within the team test's tolerance of the single call's team, with the same iterations."""
    _set_config()
    cam, kfs, cur, mps = make_world(17, n_points=1800)
    last = _last_with(kfs[0], cam, 600)
    assert last.n_features == 600
    f = dict(image=cur.mvImg_Pyr[0], levels=5, last=last, T_seed=last.Get_Pose(), align=ALIGN, min_tracked=20, keyframes=kfs,
             map_points=mps[:900])
    got = tracking.track_frames(gpu_ctx, cam, [f])[0]
    with capi.debug_options(no_team=1):
        one_cu = _single(gpu_ctx_diag, cam, f)
    _same(got, one_cu, "600 features, one CU")
    team = _single(gpu_ctx, cam, f)
    assert got["n_tracked"] == team["n_tracked"] and list(got["stats"]["iters"]) == list(team["stats"]["iters"])
    ang, dt = synth.pose_error(got["T_run"], team["T_run"])
    assert ang <= 1e-9 and dt <= 1e-9, (ang, dt)
    for r in (got, one_cu, team):
        r["frame"].close()


def _scale_frames(cam, worlds, n, nf=300):
    out = []
    for j in range(n):
        cam_, kfs, cur, mps, last = worlds[j % len(worlds)]
        out.append(dict(image=cur.mvImg_Pyr[0], levels=5, last=last, T_seed=last.Get_Pose(), align=ALIGN, min_tracked=20,
                        keyframes=kfs, map_points=mps))
    return out


@pytest.fixture(scope="module")
def scale_worlds():
    _set_config()
    ws = []
    for s in range(8):
        cam, kfs, cur, mps = make_world(500 + s, n_points=900)
        ws.append((cam, kfs, cur, mps, _last_with(kfs[0], cam, 300)))
    return ws


@pytest.mark.parametrize("n", [256, 1024])
def test_large_batches(gpu_ctx, scale_worlds, n):
    """256 and 1024 (the bound) frames of 640x480 with 300 reference features and 900 map points: sampled frames equal their single calls."""
    _set_config()
    cam = scale_worlds[0][0]
    fs = _scale_frames(cam, scale_worlds, n)
    got = tracking.track_frames(gpu_ctx, cam, fs)
    assert len(got) == n
    for j in np.random.default_rng(n).choice(n, 32, replace=False):
        want = _single(gpu_ctx, cam, fs[j])
        _same(got[j], want, f"frame {j}")
        want["frame"].close()
    assert all(len(g["matches"]) > 50 for g in got)
    for g in got:
        g["frame"].close()


def _call(ctx, cam, frames, in_grid=True):
    call = tracking.TrackBatchCall(ctx, cam, frames)
    st = call.ctx.lib.dsdtm_track_frames(call.ctx.handle, C.byref(call.cs), call.n, call.descs, call.res, call.matches.ctypes.data,
                                         call.rn.ctypes.data, call.in_grid.ctypes.data if in_grid else None)
    return st, call


def test_all_or_nothing(gpu_ctx):
    """Every error is DSDTM_ERR_INVALID before anything runs, hands out no frame, and leaves the context usable."""
    _set_config()
    cam, kfs, cur, mps = make_world(61, n_points=300)
    last = _last_with(kfs[0], cam, 150)
    base = dict(image=cur.mvImg_Pyr[0], levels=5, last=last, T_seed=last.Get_Pose(), align=ALIGN, min_tracked=20, keyframes=kfs,
                map_points=mps)
    other = capi.Context(0)
    try:
        foreign_last = Frame(cam, kfs[0].mvImg_Pyr, kfs[0].Get_Pose())
        foreign_last.set_features(last.px, last.bearing, last.p_world, last.initial)
        capi.device_frame_of(other, foreign_last)
        bad_flat = tracking.flatten_local_map(kfs, mps)
        bad_flat["okf"] = bad_flat["okf"].copy(); bad_flat["okf"][0] = 99
        cases = {
            "shared field": [dict(base), dict(base, max_matches=100)],
            "cell size": [dict(base), dict(base), dict(base, cell_size=30)],
            "bad observations in frame 2": [dict(base), dict(base), dict(base, flat=bad_flat)],
            "705 features": [dict(base), dict(base, last=_last_with(make_world(62, n_points=2000)[1][0], cam, 705))],
        }
        for what, fs in cases.items():
            if what == "705 features":
                assert fs[1]["last"].n_features == 705
            st, call = _call(gpu_ctx, cam, fs)
            assert st == capi.ERR_INVALID, what
            assert all(call.res[f].frame is None for f in range(call.n)), what
        # a reference frame / a keyframe from another context (set in the descriptors: TrackCall would upload the frame into this one)
        for field in ("ref", "kf"):
            call = tracking.TrackBatchCall(gpu_ctx, cam, [dict(base), dict(base)])
            handle = foreign_last._device_frame.handle
            if field == "ref":
                call.descs[1].ref = handle
            else:
                kfh = (C.c_void_p * len(kfs))(handle, *[capi.device_frame_of(gpu_ctx, k).handle for k in kfs[1:]])
                call.descs[1].kf = C.cast(kfh, C.c_void_p)
            st = gpu_ctx.lib.dsdtm_track_frames(gpu_ctx.handle, C.byref(call.cs), 2, call.descs, call.res, call.matches.ctypes.data,
                                                call.rn.ctypes.data, call.in_grid.ctypes.data)
            assert st == capi.ERR_INVALID and all(call.res[f].frame is None for f in range(2)), field
            assert "frame 1" in gpu_ctx.lib.dsdtm_last_error(gpu_ctx.handle).decode()
        # NULL outputs, n_frames beyond the bound, zero frames
        call = tracking.TrackBatchCall(gpu_ctx, cam, [dict(base)])
        lib, h = gpu_ctx.lib, gpu_ctx.handle
        assert lib.dsdtm_track_frames(h, C.byref(call.cs), 1, call.descs, call.res, None, call.rn.ctypes.data, None) == capi.ERR_INVALID
        assert lib.dsdtm_track_frames(h, C.byref(call.cs), 1, call.descs, None, call.matches.ctypes.data, call.rn.ctypes.data, None) == capi.ERR_INVALID
        assert lib.dsdtm_track_frames(h, C.byref(call.cs), 1025, call.descs, call.res, call.matches.ctypes.data, call.rn.ctypes.data, None) == capi.ERR_INVALID
        assert lib.dsdtm_track_frames(h, C.byref(call.cs), 0, None, None, None, None, None) == capi.OK
        assert call.res[0].frame is None
        # the context still works, and in_grid may be NULL
        st, call = _call(gpu_ctx, cam, [dict(base), dict(base)], in_grid=False)
        assert st == capi.OK and call.res[0].frame and call.res[1].frame
        for f in range(2):
            capi.DeviceFrame(gpu_ctx, C.c_void_p(call.res[f].frame)).close()
    finally:
        other.close()


def test_batch_frames_as_keyframes_and_after_their_context(gpu_ctx):
    """Frames of a batch serve as reference and keyframes of a later dsdtm_track_frame, and may be destroyed after their context."""
    _set_config()
    cam, kfs, cur, mps = make_world(71, n_points=500)
    last = _last_with(kfs[0], cam, 200)
    ctx = capi.Context(0)
    base = dict(image=cur.mvImg_Pyr[0], levels=5, last=last, T_seed=last.Get_Pose(), align=ALIGN, min_tracked=20, keyframes=kfs,
                map_points=mps)
    # the keyframes' own images through a batch: their pyramids stand in for the keyframes' and the reference frame's
    got = tracking.track_frames(ctx, cam, [dict(base, image=kf.mvImg_Pyr[0]) for kf in kfs])
    kf_b = [_as_ref(kf, g["frame"]) for kf, g in zip(kfs, got)]
    r_b = tracking.track_frame(ctx, cam, cur.mvImg_Pyr[0], 5, _as_ref(last, got[0]["frame"]), last.Get_Pose(), ALIGN, 20, kf_b, mps)
    want = tracking.track_frame(ctx, cam, cur.mvImg_Pyr[0], 5, last, last.Get_Pose(), ALIGN, 20, kfs, mps)
    _same(r_b, want, "batch frames as reference and keyframes")
    assert want["n_tracked"] > 60 and len(want["matches"]) > 30
    r_b["frame"].close(); want["frame"].close()
    handles = [g["frame"].handle for g in got]
    for g in got:
        g["frame"].handle = None
    ctx.close()
    for h in handles[::-1]:                                            # after their context: freed, not pooled
        gpu_ctx.lib.dsdtm_frame_destroy(None, h)


def test_two_contexts_on_two_threads_running_batches(gpu_ctx, scale_worlds):
    _set_config()
    cam = scale_worlds[0][0]
    fs = _scale_frames(cam, scale_worlds, 16)
    alone = tracking.track_frames(gpu_ctx, cam, fs)
    ref = [(g["T_opt"].copy(), g["matches"].copy()) for g in alone]
    for g in alone:
        g["frame"].close()
    ctxs = [capi.Context(0), capi.Context(0)]
    res = [None, None]

    def run(k):
        out = []
        for _ in range(5):
            gs = tracking.track_frames(ctxs[k], cam, fs)
            out.append([(g["T_opt"].copy(), g["matches"].copy()) for g in gs])
            for g in gs:
                g["frame"].close()
        res[k] = out

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(2):
        assert res[k] is not None
        for batch in res[k]:
            for (T, m), (Tr, mr) in zip(batch, ref):
                assert np.array_equal(T, Tr) and np.array_equal(m, mr)
    for c in ctxs:
        c.close()
