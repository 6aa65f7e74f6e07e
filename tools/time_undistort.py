"""Wall time of libdsdtm_amd_undistort.so at 640 x 480 with the map of Config/kinect.yaml, against the host functions on one thread.

    dsdtm_undistort_frames (gray + depth)   n = 1 pageable source -> device destination; n = 1, 64, 1024 device -> device
    dsdtm_undistort_points                  400 pixels for 1, 64 and 1024 trackers (one call holds at most 16384 pixels: 64 trackers are
                                            2 calls, 1024 trackers 25 calls; the time is the sum)
    where a tracker sees it                 rectify + dsdtm_frame_prefetch + dsdtm_track_frame_on against dsdtm_frame_prefetch +
                                            dsdtm_track_frame_on on the same, already rectified images — alternating in one process
    the host baseline                       tools/undistort_host_timer.cpp (undistort_frame_host / undistort_points_host, one thread,
                                            g++ -O2: this repository's own straightforward C++, not OpenCV's SIMD remap), built here

Every time is a host clock around a synchronous call (the entries wait for their stream), the median of --reps calls after a warm-up.

    python tools/time_undistort.py [--reps 200] [--out profiles/r22_undistort.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/time_undistort.py --only-kernels 200      # the kernels' device time
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINECT_CAM = (517.306408, 516.469215, 318.643040, 255.313989)
KINECT_DIST = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
W, H = 640, 480


def median_us(f, reps, warm=20):
    for _ in range(warm):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e6)
    t.sort()
    return t[len(t) // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-kernels", type=int, default=0, metavar="N", help="N calls of n = 1 and n = 64 (device to device) and of the points entry, nothing else")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from dsdtm_amd import synth, undistort
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    cam = synth.Camera(*KINECT_CAM, 525.0, W, H)
    uctx = undistort.UndistortContext(0)
    umap = uctx.make_map(cam, KINECT_DIST)
    rng = np.random.default_rng(1)
    raw, raw_z = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(400, 5000, (H, W), dtype=np.uint16)
    n_max = 64 if a.only_kernels else 1024
    src_g = torch.from_numpy(raw).cuda().repeat(n_max, 1, 1).contiguous()
    src_z = torch.from_numpy(raw_z.view(np.int16)).cuda().repeat(n_max, 1, 1).contiguous()
    dst_g, dst_z = torch.empty_like(src_g), torch.empty_like(src_z)
    torch.cuda.synchronize()

    def descs(n, pageable=False):
        fr = [dict(map=umap, gray_src=raw if pageable else src_g[i], gray_dst=dst_g[i], depth_src=raw_z if pageable else src_z[i], depth_dst=dst_z[i]) for i in range(n)]
        return uctx.descs(fr)
    px400 = np.stack([rng.uniform(0, W, 400), rng.uniform(0, H, 400)], axis=1).astype(np.float32)
    if a.only_kernels:
        for n in (1, 64):
            arr, keep = descs(n)
            for _ in range(a.only_kernels):
                uctx.check(uctx.undistort_frames_raw(n, arr))
        for _ in range(a.only_kernels):
            uctx.undistort_points(cam, KINECT_DIST, px400)
        return
    say(f"device: {torch.cuda.get_device_name(0)}; 640x480 gray + depth, the map of Config/kinect.yaml; median (min .. max) of {a.reps} calls, us")
    for label, n, pageable in (("n = 1    pageable -> device", 1, True), ("n = 1    device -> device", 1, False), ("n = 64   device -> device", 64, False),
                               ("n = 1024 device -> device", 1024, False)):
        arr, keep = descs(n, pageable)
        reps = a.reps if n < 1024 else max(10, a.reps // 10)
        med, lo, hi = median_us(lambda: uctx.check(uctx.undistort_frames_raw(n, arr)), reps, warm=5 if n == 1024 else 20)
        say(f"dsdtm_undistort_frames {label}: {med:9.1f} ({lo:.1f} .. {hi:.1f})   {med / n:8.2f} per frame")
    for trackers in (1, 64, 1024):
        px = np.tile(px400, (trackers, 1))
        chunks = [px[i:i + undistort.MAX_POINTS] for i in range(0, len(px), undistort.MAX_POINTS)]

        def run():
            for c in chunks:
                uctx.undistort_points(cam, KINECT_DIST, c)
        med, lo, hi = median_us(run, a.reps if trackers < 1024 else max(10, a.reps // 10))
        say(f"dsdtm_undistort_points {trackers:4d} x 400 ({len(chunks)} call(s), Python binding included): {med:9.1f} ({lo:.1f} .. {hi:.1f})")
    # (what a Python caller has without the device: the numpy evaluation of rule U5 — the tests' restatement, not product code)
    from dsdtm_amd import undistort_restatement as RS
    med, lo, hi = median_us(lambda: RS.undistort_points(KINECT_CAM, KINECT_DIST, px400), a.reps)
    say(f"numpy evaluation of U5, 1 x 400: {med:9.1f} ({lo:.1f} .. {hi:.1f})")
    # ---- the host baseline
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "undistort_host_timer")
        subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", os.path.join(ROOT, "tools", "undistort_host_timer.cpp"), "-o", exe], check=True)
        for ln in subprocess.run([exe, "50"], capture_output=True, text=True).stdout.splitlines():
            say("host, one thread: " + ln)
    # ---- where a tracker sees it
    from dsdtm_amd import capi, tracking
    from dsdtm_amd import undistort_restatement as R
    from dsdtm_amd.frame import Config, Frame
    from tests.test_search_gpu import make_world
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    wcam, kfs, cur, mps = make_world(11, n_points=900)
    ctx = capi.default_context(0)
    ref = kfs[0]
    nf = min(ref.n_features, 300)
    bb = ref.bearing[:nf]
    last = Frame(wcam, ref.mvImg_Pyr, ref.Get_Pose())
    last.set_features(ref.px[:nf], bb, bb * (2.0 / bb[:, 2:3]), np.ones(nf, np.uint8))
    dist = (0.05, -0.02, 0.001, -0.001, 0.0)
    wmap = uctx.make_map(wcam, dist)
    img = np.ascontiguousarray(cur.mvImg_Pyr[0])
    rect = R.remap_gray(R.undistort_map((wcam.fx, wcam.fy, wcam.cx, wcam.cy), dist, W, H), img)
    g_t = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    arr1, keep1 = uctx.descs([dict(map=wmap, gray_src=img, gray_dst=g_t)])

    def track(frame):
        call = tracking.TrackCall(ctx, wcam, None, 5, last, ref.Get_Pose(), (5, 0, 8, 15), 20, kfs, mps, cur_frame=frame)
        call.run()
        frame.close()

    def with_rectify():
        uctx.check(uctx.undistort_frames_raw(1, arr1))
        track(capi.DeviceFrame.prefetch(ctx, (g_t.data_ptr(), W, H, W), 5))

    def without():
        track(capi.DeviceFrame.prefetch(ctx, rect, 5))
    for f in (with_rectify, without):
        for _ in range(30):
            f()
    ta, tb = [], []
    for _ in range(5):                       # alternating repetitions
        ta.append(median_us(with_rectify, 60, warm=0)[0])
        tb.append(median_us(without, 60, warm=0)[0])
    say(f"per tracked frame, raw pageable image: rectify + prefetch(device) + track_frame_on {np.median(ta):.1f} us ({min(ta):.1f} .. {max(ta):.1f})")
    say(f"per tracked frame, rectified pageable image: prefetch(host) + track_frame_on        {np.median(tb):.1f} us ({min(tb):.1f} .. {max(tb):.1f})")
    say(f"the difference: {np.median(ta) - np.median(tb):+.1f} us per frame (Python adapters included in both)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
