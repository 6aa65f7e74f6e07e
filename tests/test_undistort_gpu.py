"""libdsdtm_amd_undistort.so on the MI355X: the map, the gray and depth images, the pixels and the bearings byte-equal to the restatement
(dsdtm_amd/undistort_restatement.py) on every case of tests/undistort_cases.py; a batch byte-equal to its single calls over every memory
kind; device destinations read back through torch; the hand-over to dsdtm_frame_prefetch / dsdtm_track_frame_on; the Python adapter."""
import numpy as np
import pytest

from dsdtm_amd import capi, tracking, undistort
from dsdtm_amd import undistort_restatement as R
from dsdtm_amd.frame import Config, Frame
from tests import undistort_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def uctx():
    ctx = undistort.UndistortContext(0)
    yield ctx
    ctx.close()


def _padded(h, w, stride, dtype, fill):
    buf = np.full((h, stride), fill, dtype)
    return buf, buf[:, :w]


@pytest.mark.parametrize("name", uc.FRAME_NAMES)
def test_frames_equal_the_restatement(uctx, name):
    """Pageable sources with the case's strides into padded host destinations: map, gray, depth byte-equal; the padding untouched."""
    c, want = uc.frame_case(name), uc.expected_frame(name)
    w, h = c["w"], c["h"]
    m = uctx.make_map(_cam(c), c["dist"])
    assert uc.same_bits(m.read(), want["map"])
    gbuf, gdst = _padded(h, w, c["gd"], np.uint8, 0xA5)
    f = dict(map=m, gray_src=c["gray"], gray_dst=gdst)
    if c["depth"] is not None:
        zbuf, zdst = _padded(h, w, c["zd"], np.uint16, 0xA5A5)
        f.update(depth_src=c["depth"], depth_dst=zdst)
    uctx.undistort_frames([f])
    assert uc.same_bits(gdst, want["gray"]) and (gbuf[:, w:] == 0xA5).all()
    if c["depth"] is not None:
        assert uc.same_bits(zdst, want["depth"]) and (zbuf[:, w:] == 0xA5A5).all()
    if name == "kinect_yaml":
        import hashlib
        assert hashlib.sha256(gdst.tobytes() + zdst.tobytes()).hexdigest() == uc.KINECT_SHA256
        ys, xs = np.meshgrid(np.linspace(0, 479, 8).astype(int), np.linspace(0, 639, 8).astype(int), indexing="ij")
        assert gdst[ys, xs].ravel().tolist() == uc.KINECT_SPOTS_GRAY and zdst[ys, xs].ravel().tolist() == uc.KINECT_SPOTS_DEPTH
    m.close()


class _Cam:
    def __init__(self, fx, fy, cx, cy, width, height):
        self.fx, self.fy, self.cx, self.cy, self.f, self.width, self.height = fx, fy, cx, cy, fx, width, height


def _cam(c):
    return _Cam(*c["cam"])


@pytest.mark.parametrize("name", uc.POINT_NAMES)
def test_points_equal_the_restatement(uctx, name):
    c, want = uc.point_case(name), uc.expected_points(name)
    b = np.full((len(c["px"]), 3), uc.BEARING_FILL, np.float64)
    px, b = uctx.undistort_points(_cam(c), c["dist"], c["px"], c["skip"], bearing_out=b)
    assert uc.same_bits(px, want["px"]) and uc.same_bits(b, want["bearing"])


def test_batch_mixed_equals_its_singles(uctx):
    """n = 5 over two maps: pageable, pinned and device sources; device and host destinations; gray_only and depth_given in one batch.
    Each frame is byte-equal to its single call and to the restatement; device destinations are read back through torch."""
    import torch
    names = ["gray_only", "depth_given", "barrel_strong", "tail_widths_39", "depth_given"]
    maps = {n: uctx.make_map(_cam(uc.frame_case(n)), uc.frame_case(n)["dist"]) for n in ("gray_only", "barrel_strong", "tail_widths_39")}
    maps["depth_given"] = maps["gray_only"]          # the same camera and coefficients: one map for both
    assert uc.frame_case("gray_only")["cam"] == uc.frame_case("depth_given")["cam"] and uc.frame_case("gray_only")["dist"] == uc.frame_case("depth_given")["dist"]
    kinds = [("pageable", "host"), ("pinned", "device"), ("device", "device"), ("pageable", "device"), ("device", "host")]

    def build():
        frames = []
        for name, (src_kind, dst_kind) in zip(names, kinds):
            c = uc.frame_case(name)
            h, w = c["h"], c["w"]

            def src(a):
                if a is None or src_kind == "pageable":
                    return a
                t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a))
                return t.pin_memory() if src_kind == "pinned" else t.cuda()

            def dst(dtype, fill):
                if dst_kind == "host":
                    return np.full((h, w), fill, dtype)
                return torch.full((h, w + 4), 165 if dtype == np.uint8 else -23131, dtype=torch.uint8 if dtype == np.uint8 else torch.int16, device="cuda")[:, :w]
            f = dict(map=maps[name], gray_src=src(c["gray"]), gray_dst=dst(np.uint8, 0xA5))
            if c["depth"] is not None:
                f.update(depth_src=src(c["depth"]), depth_dst=dst(np.uint16, 0xA5A5))
            frames.append(f)
        torch.cuda.synchronize()
        return frames

    def read(f):
        def host(a, dtype):
            if a is None:
                return None
            return a if isinstance(a, np.ndarray) else np.ascontiguousarray(a.cpu().numpy()).view(dtype)
        return host(f["gray_dst"], np.uint8), host(f.get("depth_dst"), np.uint16)
    batch = build()
    uctx.undistort_frames(batch)
    for name, f in zip(names, batch):
        want = uc.expected_frame(name)
        g, z = read(f)
        assert uc.same_bits(g, want["gray"]), name
        assert (z is None) == (want["depth"] is None) and (z is None or uc.same_bits(z, want["depth"])), name
    singles = build()
    for f in singles:
        uctx.undistort_frames([f])
    for a, b in zip(batch, singles):
        (ga, za), (gb, zb) = read(a), read(b)
        assert uc.same_bits(ga, gb) and (za is None or uc.same_bits(za, zb))
    # the padding of a device destination stays (rows 4 elements wider than the image)
    pad = batch[2]["gray_dst"]._base if hasattr(batch[2]["gray_dst"], "_base") and batch[2]["gray_dst"]._base is not None else None
    if pad is not None:
        assert (pad.cpu().numpy().reshape(-1, uc.frame_case("barrel_strong")["w"] + 4)[:, -4:] == 165).all()
    # refusals reach Python as UndistortError and leave the destinations alone
    bad = build()
    bad[3]["gray_dst"] = bad[3]["gray_src"]
    with pytest.raises(undistort.UndistortError, match="frame 3: gray_dst overlaps gray_src of frame 3"):
        uctx.undistort_frames(bad)
    assert (read(bad[0])[0] == 0xA5).all()
    for m in set(maps.values()):
        m.close()


def test_hand_over_to_prefetch_and_track(gpu_ctx, uctx):
    """A raw frame rectified on the device into torch tensors and prefetched from their pointers tracks to the same bits as the
    restatement's rectified images uploaded from host memory: dsdtm_track_result, matches, residual norms, and a lift of 16 pixels."""
    import torch
    from tests.test_frame_prefetch_gpu import ALIGN, LEVELS, _result_bytes
    from tests.test_search_gpu import make_world
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    cam, kfs, cur, mps = make_world(31, n_points=500, n_kf=2)
    ref = kfs[0]
    nf = min(ref.n_features, 200)
    bb = ref.bearing[:nf]
    last = Frame(cam, ref.mvImg_Pyr, ref.Get_Pose())
    last.set_features(ref.px[:nf], bb, bb * (2.0 / bb[:, 2:3]), np.ones(nf, np.uint8))
    raw = np.ascontiguousarray(cur.mvImg_Pyr[0])
    h, w = raw.shape
    raw_depth = (9000 + (uc._hash(h, w, 3) % np.uint64(2000))).astype(np.uint16)
    dist = (0.05, -0.02, 0.001, -0.001, 0.0)          # mild: a few pixels at the corners, so the tracker still tracks
    m = uctx.make_map(cam, dist)
    # path 1: device
    g_t = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    z_t = torch.empty((h, w), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    uctx.undistort_frames([dict(map=m, gray_src=raw, gray_dst=g_t, depth_src=raw_depth, depth_dst=z_t)])
    df1 = capi.DeviceFrame.prefetch(gpu_ctx, (g_t.data_ptr(), w, h, w), LEVELS, (z_t.data_ptr(), w), 5000.0)
    a = tracking.TrackCall(gpu_ctx, cam, None, LEVELS, last, ref.Get_Pose(), ALIGN, 20, kfs, mps, cur_frame=df1)
    ra = a.run()
    # path 2: the restatement's images from host memory
    rm = R.undistort_map((cam.fx, cam.fy, cam.cx, cam.cy), dist, w, h)
    g_h, z_h = R.undistort_frame(rm, raw, raw_depth)
    assert uc.same_bits(g_t.cpu().numpy(), g_h) and uc.same_bits(z_t.cpu().numpy().view(np.uint16), z_h)
    assert not np.array_equal(g_h, raw)
    df2 = capi.DeviceFrame.prefetch(gpu_ctx, g_h.copy(), LEVELS, z_h.copy(), 5000.0)
    b = tracking.TrackCall(gpu_ctx, cam, None, LEVELS, last, ref.Get_Pose(), ALIGN, 20, kfs, mps, cur_frame=df2)
    rb = b.run()
    assert _result_bytes(a) == _result_bytes(b)
    assert not ra["lost"] and ra["n_tracked"] >= 20 and rb["n_tracked"] == ra["n_tracked"]
    px = np.stack([np.linspace(30, w - 30, 16), np.linspace(25, h - 25, 16)], axis=1).astype(np.float32)
    T = np.asarray(ref.Get_Pose(), np.float64).reshape(-1)[:12]
    d1, p1 = df1.lift(cam, T, px)
    d2, p2 = df2.lift(cam, T, px)
    assert uc.same_bits(d1, d2) and uc.same_bits(p1, p2) and (d1 > 0).all()
    df1.close(); df2.close(); m.close()


def test_adapter_with_zero_distortion_leaves_the_same_keyframe_map(gpu_ctx):
    """Tracker(distortion = zeros).CraeteKeyframe against Tracker().CraeteKeyframe on two copies of one frame and two stores: the
    resident maps are byte-equal, and so are the frames (UndistortFeatures with zeros returns every pixel as it was, and the bearing of a
    feature that is not mbInitial by the rule that made it)."""
    from dsdtm_amd import keyframe_creation_restatement as KR
    from dsdtm_amd import synth, track_map
    from tests import newkf_cases
    w, h = 640, 480
    cam = synth.Camera.tum(w, h)
    rng = np.random.default_rng(34)
    tctx = track_map.TrackMapContext(0)
    T = newkf_cases.pose(rng)
    depth = newkf_cases.random_depth(rng, KR.NewKeyframeParams(w, h, 1, 1, 1, 1, 1), zeros=0.2)
    pyr = synth.build_pyramid(np.clip(np.rint(synth.make_texture(h, w, 44)), 0, 255).astype(np.uint8), 5)
    got = []
    for distortion in (None, (0.0, 0.0, 0.0, 0.0, 0.0)):
        trk = tracking.Tracker(cam, gpu_ctx, distortion=distortion)
        store, fr = track_map.TrackMapStore(tctx), Frame(cam, pyr, T.reshape(3, 4))
        out = trk.CraeteKeyframe(store, depth, cur=fr)
        m = store.map.read()
        got.append((out["n_new"], fr.px.tobytes(), fr.bearing.tobytes(), m["p_world"].tobytes(),
                    [m[k][0].tobytes() for k in ("slots", "observes", "px", "level", "bearing")]))
    assert got[0] == got[1] and got[0][0] > 20


def _track_world():
    from tests.test_search_gpu import make_world
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    cam, kfs, cur, mps = make_world(31, n_points=500, n_kf=2)
    ref = kfs[0]
    nf = min(ref.n_features, 200)
    bb = ref.bearing[:nf]
    last = Frame(cam, ref.mvImg_Pyr, ref.Get_Pose())
    last.set_features(ref.px[:nf], bb, bb * (2.0 / bb[:, 2:3]), np.ones(nf, np.uint8))
    return cam, kfs, mps, last, np.ascontiguousarray(cur.mvImg_Pyr[0])


def test_tracker_prefetch_raw_and_undistort_features(gpu_ctx):
    """Tracker.prefetch_raw with and without depth: the returned tensors are the restatement's images, TrackFrame picks the prefetched
    frame up and tracks as a plain Tracker does on the restatement's rectified image; the frame is marked rectified, so UndistortFeatures
    leaves it alone, while a frame with features detected on a raw image is moved by rule U5."""
    dist = (0.05, -0.02, 0.001, -0.001, 0.0)
    cam, kfs, mps, last, raw = _track_world()
    h, w = raw.shape
    raw_depth = (9000 + (uc._hash(h, w, 3) % np.uint64(2000))).astype(np.uint16)
    g_h, z_h = R.undistort_frame(R.undistort_map((cam.fx, cam.fy, cam.cx, cam.cy), dist, w, h), raw, raw_depth)
    trk = tracking.Tracker(cam, gpu_ctx, max_level=5, min_level=0, max_iters=8, distortion=dist)
    # without depth (the default): no depth tensor, no depth map on the frame
    raw2 = raw.copy()
    df0, g0, z0 = trk.prefetch_raw(raw2)
    assert z0 is None and uc.same_bits(g0.cpu().numpy(), g_h)
    df0.wait()
    trk._prefetched.pop()[1].close()
    # with depth
    df, g, z = trk.prefetch_raw(raw, raw_depth)
    assert uc.same_bits(g.cpu().numpy(), g_h) and uc.same_bits(z.cpu().numpy().view(np.uint16), z_h)
    cur, n, matches = trk.TrackFrame(raw, last, kfs, mps)
    assert trk._prefetched == [] and trk.last_result["frame"] is df and getattr(cur, "rectified", False)
    cam2, kfs2, mps2, last2, _ = _track_world()
    plain = tracking.Tracker(cam2, gpu_ctx, max_level=5, min_level=0, max_iters=8)
    cur2, n2, matches2 = plain.TrackFrame(g_h, last2, kfs2, mps2)
    assert n == n2 >= 20 and len(matches) == len(matches2) and not getattr(cur2, "rectified", False)
    assert np.asarray(cur.Get_Pose()).tobytes() == np.asarray(cur2.Get_Pose()).tobytes()
    assert uc.same_bits(cur.px, cur2.px) and uc.same_bits(cur.bearing, cur2.bearing)
    d1, p1 = df.lift(cam, np.asarray(last.Get_Pose(), np.float64).reshape(-1)[:12], np.array([[100.0, 80.0], [400.5, 300.25]], np.float32))
    assert (d1 > 0).all()
    # the two adapters are alternatives: a frame that came through prefetch_raw is not moved again
    px_before, b_before = cur.px.copy(), cur.bearing.copy()
    trk.UndistortFeatures(cur)
    assert uc.same_bits(cur.px, px_before) and uc.same_bits(cur.bearing, b_before)
    # features on a raw image are (the same columns, on a frame without the mark)
    fr = Frame(cam, [raw], last.Get_Pose())
    initial = (np.arange(cur.n_features) % 3 == 0).astype(np.uint8)
    fr.set_features(px_before.copy(), b_before.copy(), np.zeros((cur.n_features, 3)), initial)
    assert cur.n_features > 0
    trk.UndistortFeatures(fr)
    want_px, want_b = R.undistort_points((cam.fx, cam.fy, cam.cx, cam.cy), dist, px_before, initial, bearing_out=b_before.copy())
    assert uc.same_bits(fr.px, want_px) and uc.same_bits(fr.bearing, want_b) and not uc.same_bits(fr.px, px_before)
    trk.last_result["frame"].close(); plain.last_result["frame"].close()


def test_cpp_adapter_and_example_on_the_device(tmp_path):
    """dsdtm_amd/host/example_undistort.cpp linked and run: DSDTM::Undistorter rectifies a raw frame into device memory,
    dsdtm_frame_prefetch reads it in place, dsdtm_frame_lift and dsdtm_track_frame_on use it — it exits with 0 only when the frame, seen
    again from the same place, tracks to the identity."""
    import os
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dsdtm_amd", "host")
    exe = str(tmp_path / "example_undistort")
    subprocess.run(["g++", "-O2", "-std=c++14", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(host, "example_undistort.cpp"), undistort.lib_path(),
                    capi.lib_path(False), "-Wl,-rpath," + os.path.dirname(undistort.lib_path()), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tracked 300 of 300 features" in r.stdout and r.stdout.strip().endswith("ok"), (r.stdout, r.stderr)
