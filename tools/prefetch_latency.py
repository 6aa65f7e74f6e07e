"""Wall time per tracked frame with and without the next frame prefetched — one process, one device, the two paths alternating.

    (a) dsdtm_track_frame(image k)                                     the synchronous entry: upload + pyramid + Run + ...
    (b) dsdtm_frame_prefetch(image k + 1); dsdtm_track_frame_on(frame k)   upload + pyramid of k + 1 beside the tracking of k

on the frame bench_tracking.py's `tracked_frame` entry tracks (make_world(11, 900 points), 300 reference features, 640x480, 5
levels; the image in pageable memory, so (a) stages it in the context's block and (b) in the prefetch ring). (a) is the
yardstick: the same code as before the prefetch entries existed, measured in the same run. Per repetition the two paths run
back to back over `--frames` frames each, after a warm-up that takes the clocks out of idle; the report is the median and the
spread (min .. max) of the per-repetition medians, the gain (a) - (b), and the time of one prefetch on an otherwise idle
device (the call alone, and the call + dsdtm_frame_wait: an upper bound of the device time of the prefetch stream's kernels).

    python tools/prefetch_latency.py [--reps 5] [--frames 200] [--depth] [--out profiles/r09_prefetch.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/prefetch_latency.py --depth --only-prefetch 500    # the kernels' device time
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warm", type=int, default=300, help="frames of either path before the first repetition")
    ap.add_argument("--depth", action="store_true", help="path (b) also carries a 16-bit depth map (path (a) has no counterpart)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-prefetch", type=int, default=0, metavar="N",
                    help="N times prefetch + dsdtm_frame_wait and nothing else: the run to put under rocprofv3 --kernel-trace --stats "
                         "for the device time of the prefetch stream's kernels")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from dsdtm_amd import capi, tracking
    from dsdtm_amd.frame import Config, Frame
    from tests.test_search_gpu import make_world
    ctx = capi.default_context(0)
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    cam, kfs, cur, mps = make_world(11, n_points=900)
    L = 5
    ref = kfs[0]
    nf = min(ref.n_features, 300)
    bb = ref.bearing[:nf]
    ref_run = Frame(cam, ref.mvImg_Pyr, ref.Get_Pose())
    ref_run.set_features(ref.px[:nf], bb, bb * (2.0 / bb[:, 2:3]), np.ones(nf, np.uint8))
    seed = ref.Get_Pose().copy()
    img = np.ascontiguousarray(cur.mvImg_Pyr[0])
    d16 = (np.random.default_rng(1).integers(500, 40000, img.shape)).astype(np.uint16)
    lib, h = ctx.lib, ctx.handle
    call_a = tracking.TrackCall(ctx, cam, img, L, ref_run, seed, (L, 0, 8, 15), 20, kfs, mps)
    im = capi.FrameImage()
    im.gray, im.width, im.height, im.stride, im.levels = img.ctypes.data, cam.width, cam.height, cam.width, L
    if a.depth:
        im.depth, im.depth_stride, im.depth_scale = d16.ctypes.data, cam.width, 5000.0

    def prefetch():
        out = C.c_void_p()
        ctx.check(lib.dsdtm_frame_prefetch(h, C.byref(im), C.byref(out)))
        return out
    if a.only_prefetch:
        for _ in range(a.only_prefetch):
            f = prefetch()
            ctx.check(lib.dsdtm_frame_wait(h, f))
            lib.dsdtm_frame_destroy(h, f)
        return
    first = capi.DeviceFrame(ctx, prefetch())
    call_b = tracking.TrackCall(ctx, cam, None, L, ref_run, seed, (L, 0, 8, 15), 20, kfs, mps, cur_frame=first)
    ra, rb = call_a.run(), call_b.run()
    same = (np.array_equal(ra["T_opt"], rb["T_opt"]) and ra["matches"].tobytes() == rb["matches"].tobytes()
            and ra["residual_norm"].tobytes() == rb["residual_norm"].tobytes())
    ra["frame"].close()
    first.close()
    destroy = lib.dsdtm_frame_destroy

    def path_a(n):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            rc = call_a.run_raw()
            t1 = time.perf_counter()
            ctx.check(rc)
            destroy(h, C.c_void_p(call_a.res.frame))
            ts.append(t1 - t0)
        return ts

    def path_b(n):
        ts = []
        nxt = prefetch()
        for _ in range(n):
            curf = nxt
            t0 = time.perf_counter()
            nxt = prefetch()                                  # frame k + 1 ...
            rc = lib.dsdtm_track_frame_on(h, C.byref(call_b.cs), C.byref(call_b.desc), curf, C.byref(call_b.res),
                                          call_b.matches.ctypes.data, call_b.rn.ctypes.data)     # ... beside frame k
            t1 = time.perf_counter()
            ctx.check(rc)
            destroy(h, curf)
            ts.append(t1 - t0)
        destroy(h, nxt)
        return ts
    path_a(a.warm); path_b(a.warm)
    med_a, med_b = [], []
    for _ in range(a.reps):
        med_a.append(float(np.median(path_a(a.frames)) * 1e3))
        med_b.append(float(np.median(path_b(a.frames)) * 1e3))
    # device time of one prefetch (gray + pyramid + depth when --depth) on an idle device: wall of prefetch + wait, and the
    # host cost of the prefetch call alone
    tw, tc = [], []
    for _ in range(200):
        t0 = time.perf_counter()
        f = prefetch()
        t1 = time.perf_counter()
        ctx.check(lib.dsdtm_frame_wait(h, f))
        t2 = time.perf_counter()
        destroy(h, f)
        tc.append(t1 - t0); tw.append(t2 - t0)
    lines = [
        f"prefetch_latency: {cam.width}x{cam.height}, {L} levels, {nf} reference features, {len(mps)} map points, "
        f"{a.reps} repetitions x {a.frames} frames per path, warm-up {a.warm} frames per path, depth map on path (b): {bool(a.depth)}",
        f"device: {torch.cuda.get_device_name(0)}; library: {lib.dsdtm_version().decode()}",
        f"results of (b) equal (a) bit for bit (pose, matches, residual norms): {same}",
        "(a) dsdtm_track_frame                         wall per frame, ms: median of repetition medians "
        f"{np.median(med_a):.4f}  spread {min(med_a):.4f} .. {max(med_a):.4f}   {['%.4f' % v for v in med_a]}",
        "(b) prefetch(k+1); dsdtm_track_frame_on(k)    wall per frame, ms: median of repetition medians "
        f"{np.median(med_b):.4f}  spread {min(med_b):.4f} .. {max(med_b):.4f}   {['%.4f' % v for v in med_b]}",
        f"gain (a) - (b): {np.median(med_a) - np.median(med_b):+.4f} ms; spread of the repetitions: (a) {max(med_a) - min(med_a):.4f} ms, "
        f"(b) {max(med_b) - min(med_b):.4f} ms",
        f"one prefetch on an idle device, ms: host cost of the call, median {np.median(tc) * 1e3:.4f}; call + dsdtm_frame_wait, median "
        f"{np.median(tw) * 1e3:.4f} (upper bound of the device time of the prefetch stream's kernels for one frame)",
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
