"""dsdtm_frame_prefetch / dsdtm_frame_wait / dsdtm_track_frame_on / dsdtm_frame_lift — an RGB-D frame enters the device once,
ahead of time (reference src/Frame.cpp:35-41, src/Tracking.cpp:56-57), and Frame::Get_FeatureDetph + Frame::UnProject
(src/Frame.cpp:152-157, 201-224) are a query on the resident frame. Held to
  * dsdtm_frame_create_from_image, byte for byte, on every way an image can arrive;
  * dsdtm_track_frame on the same descriptor, bit for bit, single frames and a tracked sequence with frame k + 1 prefetched
    before frame k is tracked;
  * tum.depth_to_metres / tum.get_feature_depth (float-equal) and tests/rgbd_restatement.py (4 ulp) for the depth half;
  * the C ABI's argument checks."""
import copy
import ctypes as C

import numpy as np
import pytest

from dsdtm_amd import capi, search, synth, tracking, tum
from dsdtm_amd.frame import Config, Frame
from dsdtm_amd.sparse_align import Sprase_ImgAlign
from tests import rgbd_restatement as R
from tests.test_search_gpu import make_world

pytestmark = pytest.mark.gpu

LEVELS = 5
ALIGN = (5, 0, 8, 15)


# ---- reading a frame back -------------------------------------------------------------------------------------------
_HIP = []


def _hip():
    """The HIP runtime this process already runs on (the one libdsdtm_amd.so is bound to), for hipMemcpy."""
    if not _HIP:
        capi.load()
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "libamdhip64 is not mapped into this process"
        lib = C.CDLL(path)
        lib.hipMemcpy.restype = C.c_int
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.append(lib)
    return _HIP[0]


class _FrameHead(C.Structure):
    """The first members of struct dsdtm_frame (dsdtm_amd/csrc/api_internal.h): owner, device, d (the packed pyramid), pitch."""
    _fields_ = [("owner", C.c_void_p), ("device", C.c_int), ("d", C.c_void_p), ("pitch", C.c_size_t)]


def pyramid_levels(df, width, height, levels=LEVELS):
    """The frame's pyramid as a list of (h, w) uint8 arrays, copied back from the device (the caller has waited for the frame)."""
    head = _FrameHead.from_address(df.handle.value)
    ws, hs, _, offs, total = capi.pyramid_layout(width, height, levels)
    assert head.pitch == (total + 255) // 256 * 256
    buf = np.empty(total, np.uint8)
    assert _hip().hipMemcpy(buf.ctypes.data, head.d, total, 2) == 0          # 2 = hipMemcpyDeviceToHost
    return [buf[offs[l]:offs[l] + ws[l] * hs[l]].reshape(hs[l], ws[l]).copy() for l in range(levels)]


def same_pyramid(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def make_image(width, height, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    return ((xx * 3 + yy * 5 + rng.integers(0, 64, (height, width))) % 256).astype(np.uint8)


# ---- 1. every way the image can arrive ---------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(640, 480), (636, 478)])
def test_every_way_the_image_can_arrive_gives_the_frame_of_create_from_image(gpu_ctx, oracle, width, height):
    """Pageable (staged in the prefetch ring), pinned and 16-byte aligned (read in place by the ingest kernel), pinned at an odd
    address (the copy engine), row-strided (pageable and pinned: packed into the ring), device-resident (in place; strided: a
    device-to-device copy). 636 x 478: the byte count is no multiple of 16 (the kernel's byte tail) and the level widths are
    no multiples of 8 (one pyrDown launch per level)."""
    import torch
    img = make_image(width, height, 5)
    n = width * height
    assert (n % 16 == 0) == (width == 640)
    ref = capi.DeviceFrame.from_image(gpu_ctx, img, LEVELS)
    want = pyramid_levels(ref, width, height)
    assert np.array_equal(want[0], img)
    chain = [img]
    for _ in range(1, LEVELS):
        chain.append(oracle.pyrdown(chain[-1]))
    assert same_pyramid(want, chain), "the pyramid of create_from_image is not the oracle's chain"
    pin = torch.empty(n + 64, dtype=torch.uint8).pin_memory()
    pin_s = torch.empty(height * (width + 24), dtype=torch.uint8).pin_memory()
    flat = pin.numpy()
    assert flat.ctypes.data % 16 == 0
    aligned = flat[:n].reshape(height, width)
    odd = flat[4:4 + n].reshape(height, width)
    strided = pin_s.numpy().reshape(height, width + 24)[:, :width]; strided[:] = img
    pageable_strided = np.zeros((height, width + 7), np.uint8)[:, :width]; pageable_strided[:] = img
    dev = torch.from_numpy(img).cuda()
    dev_s = torch.zeros((height, width + 40), dtype=torch.uint8, device="cuda"); dev_s[:, :width] = dev
    torch.cuda.synchronize()

    def check(name, src):
        df = capi.DeviceFrame.prefetch(gpu_ctx, src, LEVELS)
        df.wait()
        assert same_pyramid(pyramid_levels(df, width, height), want), name
        df.close()
    check("pageable", img.copy())
    aligned[:] = img
    check("pinned, aligned", aligned)
    odd[:] = img                                            # (shares the buffer with `aligned`, which has been waited for)
    assert odd.ctypes.data % 16 == 4
    check("pinned, odd address", odd)
    check("pinned, row-strided", strided)
    check("pageable, row-strided", pageable_strided)
    assert dev.data_ptr() % 16 == 0
    check("device", (dev.data_ptr(), width, height, width))
    check("device, row-strided", (dev_s.data_ptr(), width, height, width + 40))
    ref.close()


# ---- 2. / 3. tracking on a prefetched frame ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    cam, kfs, cur, mps = make_world(31, n_points=500, n_kf=2)
    ref = kfs[0]
    nf = min(ref.n_features, 200)
    bb = ref.bearing[:nf]
    last = Frame(cam, ref.mvImg_Pyr, ref.Get_Pose())
    last.set_features(ref.px[:nf], bb, bb * (2.0 / bb[:, 2:3]), np.ones(nf, np.uint8))
    return cam, kfs, np.ascontiguousarray(cur.mvImg_Pyr[0]), mps, last, ref


def _result_bytes(call):
    """Every field of dsdtm_track_result behind `frame`, the match list and the residual norms, as raw bytes."""
    res = call.res
    n_rn = res.summary.n_residual_blocks
    return (bytes(res)[capi.TrackResult.T_run.offset:], call.matches[:res.n_matches].tobytes(), call.rn[:n_rn].tobytes())


@pytest.mark.parametrize("case", ["standard", "lost", "empty local map"])
def test_track_frame_on_equals_track_frame_bit_for_bit(gpu_ctx, world, case):
    cam, kfs, img, mps, last, ref = world
    min_tracked = 100000 if case == "lost" else 20
    k_, m_ = ([], []) if case == "empty local map" else (kfs, mps)
    a = tracking.TrackCall(gpu_ctx, cam, img, LEVELS, last, ref.Get_Pose(), ALIGN, min_tracked, k_, m_)
    ra = a.run()
    df = capi.DeviceFrame.prefetch(gpu_ctx, img.copy(), LEVELS)                      # pending when the call below starts
    b = tracking.TrackCall(gpu_ctx, cam, None, LEVELS, last, ref.Get_Pose(), ALIGN, min_tracked, k_, m_, cur_frame=df)
    rb = b.run()
    assert b.res.frame == df.handle.value and rb["frame"] is df
    assert _result_bytes(a) == _result_bytes(b)
    assert ra["n_tracked"] >= 100
    assert ra["lost"] == (case == "lost") and (len(ra["matches"]) >= 40) == (case == "standard")
    assert same_pyramid(pyramid_levels(df, cam.width, cam.height), pyramid_levels(ra["frame"], cam.width, cam.height))
    # a settled frame, and one from dsdtm_frame_create_from_image, give the same again
    c = tracking.TrackCall(gpu_ctx, cam, None, LEVELS, last, ref.Get_Pose(), ALIGN, min_tracked, k_, m_, cur_frame=df)
    c.run()
    fi = capi.DeviceFrame.from_image(gpu_ctx, img, LEVELS)
    e = tracking.TrackCall(gpu_ctx, cam, None, LEVELS, last, ref.Get_Pose(), ALIGN, min_tracked, k_, m_, cur_frame=fi)
    e.run()
    assert _result_bytes(c) == _result_bytes(a) and _result_bytes(e) == _result_bytes(a)
    for f in (ra["frame"], df, fi):
        f.close()


def test_sequence_with_the_next_frame_prefetched_equals_track_frame(gpu_ctx):
    """Seven frames tracked twice on copies of one world: through dsdtm_track_frame, and with prefetch(k + 1) issued BEFORE
    track_frame_on(k). The caller's (pageable, hence staged) buffer is overwritten with 0xFF as soon as each prefetch has
    returned: the staging contract. Poses, match lists and residual norms per frame are the same bits — frame k is the
    reference frame of frame k + 1, so a difference would also compound."""
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    n_kf, n_frames = 2, 7
    cam, kfs, _, mps = make_world(21, n_points=700, n_kf=n_kf)
    rng = np.random.default_rng(77)
    tex = synth.make_texture(cam.height, cam.width, 21)
    for k, kf in enumerate(kfs):
        mpts = [None] * kf.n_features
        for mp in mps:
            if k in mp.mObservations:
                mpts[mp.mObservations[k]] = mp
        kf.mvMapPoints = mpts
        kf.p_world = np.array([m_.mPose if m_ is not None else np.zeros(3) for m_ in mpts])
        kf.initial = np.array([1 if m_ is not None else 0 for m_ in mpts], np.uint8)
    worlds = [copy.deepcopy((kfs, mps)) for _ in range(2)]
    T0 = np.vstack([kfs[n_kf - 1].Get_Pose(), [0, 0, 0, 1]])
    imgs, xi = [], np.zeros(6)
    for k in range(n_frames):
        xi = xi + np.concatenate([rng.uniform(-0.012, 0.012, 3), rng.uniform(-0.006, 0.006, 3)])
        imgs.append(synth.warp_plane(tex, cam, synth.se3_exp(xi) @ T0, 2.0))
    align = (5, 0, 8, int(Config.Get("Camera.Min_fts")))

    a_kfs, a_mps = worlds[0]
    log, last = [], a_kfs[n_kf - 1]
    for k in range(n_frames):
        r = tracking.track_frame(gpu_ctx, cam, imgs[k], LEVELS, last, last.Get_Pose(), align, 20, a_kfs, a_mps)
        log.append(r)
        last, _, _ = tracking.apply_tracked_frame(cam, imgs[k], r, a_mps)

    b_kfs, b_mps = worlds[1]
    last = b_kfs[n_kf - 1]

    def send(k):
        buf = imgs[k].copy()
        df = capi.DeviceFrame.prefetch(gpu_ctx, buf, LEVELS)
        buf[:] = 0xFF                                       # staged: the buffer is the caller's again
        return df
    nxt = send(0)
    for k in range(n_frames):
        cur_frame, nxt = nxt, (send(k + 1) if k + 1 < n_frames else None)
        r = tracking.track_frame(gpu_ctx, cam, None, LEVELS, last, last.Get_Pose(), align, 20, b_kfs, b_mps, cur_frame=cur_frame)
        a = log[k]
        assert r["n_tracked"] == a["n_tracked"] and r["stats"] == a["stats"] and r["lost"] == a["lost"], k
        assert np.array_equal(r["T_run"], a["T_run"]) and np.array_equal(r["T_opt"], a["T_opt"]), f"frame {k}: poses"
        assert r["matches"].tobytes() == a["matches"].tobytes() and len(r["matches"]) >= 60, f"frame {k}: match list"
        assert r["residual_norm"].tobytes() == a["residual_norm"].tobytes(), f"frame {k}: residual norms"
        last, _, _ = tracking.apply_tracked_frame(cam, imgs[k], r, b_mps)
    assert log[-1]["n_tracked"] >= 40


def test_tracker_prefetch_then_trackframe(gpu_ctx, world):
    """tracking.Tracker: prefetch(image) then TrackFrame(image) runs on the prefetched frame and gives TrackFrame's results."""
    cam, kfs, img, mps, last, ref = world
    t = tracking.Tracker(cam, ctx=gpu_ctx, max_level=5, min_level=0, max_iters=8, min_tracked=20)
    cur_a, n_a, m_a = t.TrackFrame(img, last, kfs, copy.deepcopy(mps))
    ra = t.last_result
    df = t.prefetch(img)
    cur_b, n_b, m_b = t.TrackFrame(img, last, kfs, copy.deepcopy(mps))
    rb = t.last_result
    assert rb["frame"] is df and not t._prefetched
    # frames the caller prefetched and then skipped are released, not kept at the head for good
    other = [img.copy() for _ in range(3)]
    s0, s1 = t.prefetch(other[0]), t.prefetch(other[1])
    s2 = t.prefetch(other[2])                                   # a third: the oldest goes
    assert s0.handle is None and [d_ for _, d_ in t._prefetched] == [s1, s2]
    t.TrackFrame(other[2], last, kfs, copy.deepcopy(mps))
    assert t.last_result["frame"] is s2 and s1.handle is None and not t._prefetched
    assert t.last_result["matches"].tobytes() == ra["matches"].tobytes()
    assert n_a == n_b and np.array_equal(cur_a.Get_Pose(), cur_b.Get_Pose()) and ra["matches"].tobytes() == rb["matches"].tobytes()


# ---- 4. ring and pool --------------------------------------------------------------------------------------------------
def test_ring_slot_reuse_and_a_pending_frame_destroyed(gpu_ctx):
    """Three staged prefetches in a row with no consumer between them: the third re-uses the first one's slot of the two-slot
    ring. Then a pending frame is destroyed (its buffer goes to the pool with its event) and another frame of the same size is
    prefetched into that buffer. Every pyramid that is left must be right."""
    w, h = 320, 240
    imgs = [make_image(w, h, 40 + i) for i in range(5)]
    refs = [capi.DeviceFrame.from_image(gpu_ctx, im, LEVELS) for im in imgs]
    want = [pyramid_levels(r, w, h) for r in refs]
    for r in refs:
        r.close()
    bufs = [im.copy() for im in imgs]
    fr = []
    for i in range(3):
        fr.append(capi.DeviceFrame.prefetch(gpu_ctx, bufs[i], LEVELS))
        bufs[i][:] = 0xFF
    fr.append(capi.DeviceFrame.prefetch(gpu_ctx, bufs[3], LEVELS))
    fr[3].close()                                           # pending (or not): legal either way
    fr[3] = None
    fr.append(capi.DeviceFrame.prefetch(gpu_ctx, bufs[4], LEVELS))
    for i in (4, 0, 2, 1):                                  # (waiting for a later frame settles the earlier ones)
        fr[i].wait()
        assert same_pyramid(pyramid_levels(fr[i], w, h), want[i]), i
    # a pooled buffer taken by a frame that is NOT prefetched (the compute stream waits for the event behind it)
    p = capi.DeviceFrame.prefetch(gpu_ctx, imgs[0].copy(), LEVELS)
    p.close()
    q = capi.DeviceFrame.from_image(gpu_ctx, imgs[1], LEVELS)
    assert same_pyramid(pyramid_levels(q, w, h), want[1])
    for f in fr + [q]:
        if f is not None:
            f.close()


# ---- 5. a pending frame as ref / kf ------------------------------------------------------------------------------------
def test_a_pending_frame_as_ref_and_as_keyframe(gpu_ctx, world):
    cam, kfs, img, mps, last, ref = world
    cur = Frame(cam, synth.build_pyramid(img, 5), ref.Get_Pose())
    cur_d = capi.device_frame_of(gpu_ctx, cur)
    al = Sprase_ImgAlign(5, 0, 8, ctx=gpu_ctx, resident_frames=True)

    def run_align(ref_frame_device):
        lf = Frame(cam, ref.mvImg_Pyr, ref.Get_Pose())
        lf.set_features(last.px, last.bearing, last.p_world, last.initial)
        lf._device_frame = ref_frame_device
        c = Frame(cam, cur.mvImg_Pyr, ref.Get_Pose())
        c._device_frame = cur_d
        n = al.Run(c, lf)
        return n, c.Get_Pose().copy(), list(al.last_stats["iters"])
    img0 = np.ascontiguousarray(ref.mvImg_Pyr[0])
    want = run_align(capi.DeviceFrame.from_image(gpu_ctx, img0, LEVELS))
    got = run_align(capi.DeviceFrame.prefetch(gpu_ctx, img0.copy(), LEVELS))      # pending
    assert want[0] >= 100 and got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] == want[2]

    def run_search(pending):
        ks = [copy.copy(k) for k in kfs]                    # (shallow: the same images and features, a device frame of their own)
        for k in ks:
            l0 = np.ascontiguousarray(k.mvImg_Pyr[0])
            k._device_frame = capi.DeviceFrame.prefetch(gpu_ctx, l0.copy(), LEVELS) if pending else capi.DeviceFrame.from_image(gpu_ctx, l0, LEVELS)
        ms = copy.deepcopy(mps)
        c = Frame(cam, cur.mvImg_Pyr, kfs[-1].Get_Pose())
        c._device_frame = cur_d
        s = search.LocalPointSearch(cam, ctx=gpu_ctx, resident_frames=True)
        s.ResetGrid()
        for mp in ms:
            if not mp.IsBad():
                s.ReprojectPoint(c, mp)
        idx = {id(mp): i for i, mp in enumerate(ms)}
        return [(g[0], idx[id(g[1])], float(g[2][0]), float(g[2][1]), g[3]) for g in s.SearchLocalPoints(c, ks)]
    want = run_search(False)
    got = run_search(True)
    assert got == want and len(want) >= 20


# ---- 6. / 7. depth -----------------------------------------------------------------------------------------------------
def depth_map(width, height, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(300, 40000, (height, width)).astype(np.uint16)
    d[rng.random((height, width)) < 0.15] = 0                       # holes
    d[height // 3:height // 3 + 6, width // 4:width // 4 + 9] = 0   # a hole larger than the neighbourhood: pixels with no depth at all
    d[0, 0], d[0, -1], d[-1, 0], d[-1, -1] = 0, 65535, 65535, 0
    d[1, 0] = d[0, 1] = 0                                           # corner (0, 0): every neighbour inside the image is a hole too
    d[height // 2, width // 2] = 65535
    return d


def expected_depths(plane):
    """tum.get_feature_depth at every integer pixel, vectorised: the pixel, else the first non-zero of (-1,0), (0,-1), (1,0), (0,1)."""
    h, w = plane.shape
    pad = np.zeros((h + 2, w + 2), np.float32)
    pad[1:-1, 1:-1] = plane
    out = np.full((h, w), -1.0, np.float32)
    for dx, dy in ((0, 1), (1, 0), (0, -1), (-1, 0), (0, 0)):       # reversed priority: the later assignment wins
        nb = pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        out = np.where(nb != 0, nb, out)
    return out


def lift_all(df, cam, T, px):
    d, p = [], []
    for i in range(0, len(px), capi.LIFT_MAX):
        a, b = df.lift(cam, T, px[i:i + capi.LIFT_MAX])
        d.append(a); p.append(b)
    return np.concatenate(d), np.concatenate(p)


@pytest.mark.parametrize("width,height,stride,scale,memory", [
    (64, 48, 64, 5000.0, "pageable"), (64, 48, 64, 1000.0, "pinned"), (64, 48, 64, 5000.0, "device"),
    (68, 48, 72, 1000.0, "pinned"), (637, 479, 650, 5000.0, "pageable"), (637, 479, 650, 1000.0, "pinned")])
def test_depth_plane_equals_depth_to_metres_at_every_pixel(gpu_ctx, width, height, stride, scale, memory):
    """The frame's float plane, read back through the lift at every integer pixel. 64 wide: whole 16-byte pieces; 68 wide with
    rows 72 apart: pieces and a scalar tail, rows strided in place; 637: odd width, scalar throughout. Pageable maps are staged,
    pinned and device ones read in place."""
    import torch
    d16 = depth_map(width, height, 3 + width)
    if memory == "pinned":
        t = torch.empty(height * stride, dtype=torch.int16).pin_memory()
        src = t.numpy().view(np.uint16).reshape(height, stride)[:, :width]; src[:] = d16
    elif memory == "device":
        t = torch.from_numpy(d16.view(np.int16)).cuda(); torch.cuda.synchronize()
        src = (t.data_ptr(), width)
    else:
        src = np.zeros((height, stride), np.uint16)[:, :width]; src[:] = d16
    cam = synth.Camera.tum(width, height)
    df = capi.DeviceFrame.prefetch(gpu_ctx, make_image(width, height, 1), 2, depth=src, depth_scale=scale)
    plane = tum.depth_to_metres(d16, scale)
    yy, xx = np.mgrid[0:height, 0:width]
    px = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.float32)
    T = np.eye(4)[:3]
    got, pts = lift_all(df, cam, T, px)
    got = got.reshape(height, width)
    assert np.array_equal(got[d16 != 0].view(np.uint32), plane[d16 != 0].view(np.uint32))       # bit for bit
    want = expected_depths(plane)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (want == -1).sum() >= 4 and (d16 == 0).sum() > (want == -1).sum()
    holes = np.argwhere(d16 == 0)[:400]
    for y, x in holes:                                                                           # the vectorised rule against tum's
        assert want[y, x] == np.float32(tum.get_feature_depth(plane, (np.float32(x), np.float32(y))))
    assert np.all(pts.reshape(height, width, 3)[want == -1] == 0)
    df.close()


def test_lift_equals_the_restatement(gpu_ctx):
    width, height, scale = 64, 48, 5000.0
    d16 = np.full((height, width), 0, np.uint16)
    rng = np.random.default_rng(9)
    d16[:] = rng.integers(2000, 30000, (height, width))
    # holes whose only non-zero neighbour is each of the four in turn, and one with none
    centres = {"left": (10, 10), "up": (20, 10), "right": (30, 10), "down": (40, 10), "none": (50, 10)}
    for name, (x, y) in centres.items():
        d16[y - 1:y + 2, x - 1:x + 2] = 0
        if name != "none":
            dx, dy = {"left": (-1, 0), "up": (0, -1), "right": (1, 0), "down": (0, 1)}[name]
            d16[y + dy, x + dx] = 12345 + x
    d16[0, 0] = d16[0, 1] = d16[1, 0] = 0                           # corner: the neighbours outside have no depth, those inside are holes
    d16[0, 30] = 0; d16[height - 1, 30] = 0; d16[20, 0] = 0; d16[20, width - 1] = 0     # edge holes
    d16[height - 1, width - 1] = 0; d16[height - 2, width - 1] = 0; d16[height - 1, width - 2] = 0
    plane = tum.depth_to_metres(d16, scale)
    cam = synth.Camera.tum(width, height)
    px = [(x, y) for x, y in centres.values()]
    px += [(0, 0), (30, 0), (30, height - 1), (0, 20), (width - 1, 20), (width - 1, height - 1), (width - 1, 0), (0, height - 1)]
    for k in (6, 7, 21, 22):                                         # k + 0.5 -/+ 1e-4 in both parities: cvRound's ties go to even
        for e in (-1e-4, 0.0, 1e-4):
            px += [(k + 0.5 + e, 5.0), (5.0, k + 0.5 + e), (k + 0.5 + e, k + 0.5 - e)]
    px += [(-0.4, 3.0), (-0.6, 3.0), (width - 0.6, 3.0), (width - 0.4, 3.0), (3.0, height - 0.4), (3.0, -0.6), (1e6, 1e6), (-1e6, 5.0)]
    px += [tuple(v) for v in rng.uniform(0, [width - 1, height - 1], (300, 2))]
    px = np.array(px, np.float32)
    T = (synth.se3_exp(np.array([0.5, -0.6, 0.62, 0.3, -0.2, 0.45])))[:3]           # a real rotation, |t| ~ 1
    assert 0.9 < np.linalg.norm(T[:, 3]) < 1.1 and abs(T[0, 1]) > 0.1
    df = capi.DeviceFrame.prefetch(gpu_ctx, make_image(width, height, 2), 2, depth=d16, depth_scale=scale)
    got_d, got_p = df.lift(cam, T, px)
    want_d, want_p = R.lift(plane, cam, T, px)
    assert np.array_equal(got_d.view(np.uint32), want_d.view(np.uint32))                                  # float-equal, the -1s included
    for name, (x, y) in centres.items():
        i = list(centres).index(name)
        assert (got_d[i] == -1) == (name == "none") and (name == "none" or got_d[i] == plane[y + {"left": 0, "up": -1, "right": 0, "down": 1}[name],
                                                                                                 x + {"left": -1, "up": 0, "right": 1, "down": 0}[name]])
    assert (got_d == -1).sum() >= 8 and (got_d != -1).sum() >= 300
    # non-finite coordinates have no depth (cvRound gives INT_MIN for them; tum.cv_round cannot take them)
    bad = np.array([[np.nan, 5.0], [5.0, np.nan], [np.inf, 5.0], [5.0, -np.inf], [np.nan, np.nan]], np.float32)
    bad_d, bad_p = df.lift(cam, T, bad)
    assert np.all(bad_d == -1) and np.all(bad_p == 0)
    err, worst = 0.0, 0.0
    for i in range(len(px)):
        if want_d[i] == -1:
            assert np.all(got_p[i] == 0)
            continue
        d = float(want_d[i])
        p_c = max(abs(d * (float(px[i, 0]) - cam.cx) / cam.fx), abs(d * (float(px[i, 1]) - cam.cy) / cam.fy), d)
        bound = R.ulp_bound(p_c, float(np.abs(T[:, 3]).max()))
        e = float(np.abs(got_p[i] - want_p[i]).max())
        worst = max(worst, e / bound)
        err = max(err, e)
    print(f"lift: largest |difference| {err:.3e}, largest difference / (4 ulp bound) {worst:.3f}")
    assert worst <= 1.0
    df.close()


# ---- 8. argument errors ------------------------------------------------------------------------------------------------
def test_argument_errors_name_the_field_and_leave_the_context_usable(gpu_ctx, world):
    cam, kfs, img, mps, last, ref = world
    lib, ctx = gpu_ctx.lib, gpu_ctx

    def err():
        return lib.dsdtm_last_error(ctx.handle).decode()
    df = capi.DeviceFrame.prefetch(ctx, img.copy(), LEVELS)
    # image != NULL in track_frame_on
    call = tracking.TrackCall(ctx, cam, None, LEVELS, last, ref.Get_Pose(), ALIGN, 20, kfs, mps, cur_frame=df)
    keep = img.copy()
    call.desc.image = keep.ctypes.data
    assert call.run_raw() == capi.ERR_INVALID and "image" in err()
    call.desc.image = None
    # a size mismatch
    call.desc.levels = 4
    assert call.run_raw() == capi.ERR_INVALID and "levels" in err()
    call.desc.levels = LEVELS
    small = capi.DeviceFrame.prefetch(ctx, make_image(320, 240, 1), LEVELS)
    call.cur_frame = small
    assert call.run_raw() == capi.ERR_INVALID and "width" in err()
    call.cur_frame = df
    # NULL pointers
    cs = capi.camera_struct(cam)
    assert lib.dsdtm_track_frame_on(ctx.handle, C.byref(cs), C.byref(call.desc), None, C.byref(call.res), call.matches.ctypes.data,
                                    call.rn.ctypes.data) == capi.ERR_INVALID and "cur" in err()
    out = C.c_void_p()
    assert lib.dsdtm_frame_prefetch(ctx.handle, None, C.byref(out)) == capi.ERR_INVALID and "image" in err()
    im = capi.FrameImage()
    im.width, im.height, im.stride, im.levels = cam.width, cam.height, cam.width, LEVELS
    assert lib.dsdtm_frame_prefetch(ctx.handle, C.byref(im), C.byref(out)) == capi.ERR_INVALID and "gray" in err() and not out.value
    im.gray = keep.ctypes.data
    assert lib.dsdtm_frame_prefetch(ctx.handle, C.byref(im), None) == capi.ERR_INVALID and "out" in err()
    im.stride = cam.width - 1
    assert lib.dsdtm_frame_prefetch(ctx.handle, C.byref(im), C.byref(out)) == capi.ERR_INVALID and "stride" in err()
    im.stride = cam.width
    d16 = np.ones((cam.height, cam.width), np.uint16)
    im.depth, im.depth_stride, im.depth_scale = d16.ctypes.data, cam.width, 0.0
    assert lib.dsdtm_frame_prefetch(ctx.handle, C.byref(im), C.byref(out)) == capi.ERR_INVALID and "depth_scale" in err()
    assert lib.dsdtm_frame_wait(ctx.handle, None) == capi.ERR_INVALID and "frame" in err()
    # lift: a frame without depth, n over the limit, NULL pointers
    px = np.zeros((capi.LIFT_MAX + 1, 2), np.float32)
    dd = np.zeros(capi.LIFT_MAX + 1, np.float32)
    pp = np.zeros((capi.LIFT_MAX + 1, 3))
    T = np.ascontiguousarray(np.eye(4)[:3].reshape(12))
    args = lambda f, n, a=px, b=dd, c=pp, t=T: (ctx.handle, f, C.byref(cs), t.ctypes.data if t is not None else None,
                                               a.ctypes.data if a is not None else None, n, b.ctypes.data if b is not None else None,
                                               c.ctypes.data if c is not None else None)
    assert lib.dsdtm_frame_lift(*args(df.handle, 4)) == capi.ERR_INVALID and "depth" in err()
    dfd = capi.DeviceFrame.prefetch(ctx, img.copy(), LEVELS, depth=d16, depth_scale=5000.0)
    assert lib.dsdtm_frame_lift(*args(dfd.handle, capi.LIFT_MAX + 1)) == capi.ERR_INVALID and "n =" in err()
    assert lib.dsdtm_frame_lift(*args(None, 4)) == capi.ERR_INVALID and "frame" in err()
    assert lib.dsdtm_frame_lift(*args(dfd.handle, 4, a=None)) == capi.ERR_INVALID and "px_xy" in err()
    assert lib.dsdtm_frame_lift(*args(dfd.handle, 4, b=None)) == capi.ERR_INVALID and "depth_out" in err()
    assert lib.dsdtm_frame_lift(*args(dfd.handle, 4, c=None)) == capi.ERR_INVALID and "p_world_out" in err()
    assert lib.dsdtm_frame_lift(*args(dfd.handle, 4, t=None)) == capi.ERR_INVALID and "T_c2w" in err()
    # the context still works: the limit itself, and the tracked frame
    assert lib.dsdtm_frame_lift(*args(dfd.handle, capi.LIFT_MAX)) == capi.OK and np.all(dd[:capi.LIFT_MAX] == tum.depth_to_metres(np.ones(1, np.uint16), 5000.0)[0])
    r = call.run()
    assert r["n_tracked"] >= 100 and r["frame"] is df
    for f in (df, small, dfd):
        f.close()
