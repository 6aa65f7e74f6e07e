"""Tracked frames per second through dsdtm_track_frames (one call = n frames of n independent trackers) against dsdtm_track_frame
(one call per frame: 1 context on 1 thread, and 16 contexts on 16 threads).

    python tools/track_batch_rate.py [--n 1,16,64,256,1024] [--reps 20] [--threads 16] [--only-batch N]

World: 640x480, 300 reference features and 900 map points per frame (8 distinct worlds, repeated). Images either in device
memory (a torch tensor per frame) or in pinned host memory. Prints one line per configuration and a JSON summary at the end.
`--only-batch N` runs just the device-image batch of N frames (for a rocprofv3 --kernel-trace --stats run of the stages)."""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from dsdtm_amd import capi, tracking  # noqa: E402
from dsdtm_amd.frame import Config, Frame  # noqa: E402
from tests.test_search_gpu import make_world  # noqa: E402


def worlds(k=8):
    Config.Set("Camera.CellSize", 25); Config.Set("Camera.MaxPyraLevels", 5); Config.Set("Camera.Min_fts", 15)
    out = []
    for s in range(k):
        cam, kfs, cur, mps = make_world(500 + s, n_points=900)
        ref = kfs[0]
        nf = 300
        bb = ref.bearing[:nf]
        last = Frame(cam, ref.mvImg_Pyr, ref.Get_Pose())
        last.set_features(ref.px[:nf], bb, bb * (2.0 / bb[:, 2:3]), np.ones(nf, np.uint8))
        out.append((cam, kfs, cur, mps, last))
    return out


def frames_of(ws, n, images):
    return [dict(image=images[j % len(ws)], levels=5, last=ws[j % len(ws)][4], T_seed=ws[j % len(ws)][4].Get_Pose(), align=(5, 0, 8, 15),
                 min_tracked=20, keyframes=ws[j % len(ws)][1], map_points=ws[j % len(ws)][3]) for j in range(n)]


def point_images(call, ptrs):
    for f in range(call.n):
        call.descs[f].image = ptrs[f % len(ptrs)]


def time_batch(ctx, cam, ws, n, ptrs, reps):
    call = tracking.TrackBatchCall(ctx, cam, frames_of(ws, n, [w[2].mvImg_Pyr[0] for w in ws]))
    point_images(call, ptrs)
    lib = ctx.lib

    def once():
        ctx.check(call.run_raw())
        for f in range(n):
            lib.dsdtm_frame_destroy(ctx.handle, call.res[f].frame)
    for _ in range(3):
        once()
    t0 = time.perf_counter()
    for _ in range(reps):
        once()
    dt = (time.perf_counter() - t0) / reps
    return dt


def time_single(ctxs, cam, ws, ptrs, reps):
    calls = []
    for k, ctx in enumerate(ctxs):
        w = ws[k % len(ws)]
        c = tracking.TrackCall(ctx, cam, w[2].mvImg_Pyr[0], 5, w[4], w[4].Get_Pose(), (5, 0, 8, 15), 20, w[1], w[3])
        c.desc.image = ptrs[k % len(ptrs)]
        calls.append(c)

    def loop(c, m):
        for _ in range(m):
            c.ctx.check(c.run_raw())
            c.ctx.lib.dsdtm_frame_destroy(c.ctx.handle, c.res.frame)
    for c in calls:
        loop(c, 5)
    th = [threading.Thread(target=loop, args=(c, reps)) for c in calls]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = time.perf_counter() - t0
    return len(calls) * reps / dt, dt / reps


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,16,64,256,1024")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--only-batch", type=int, default=0)
    a = ap.parse_args()
    ws = worlds()
    cam = ws[0][0]
    ctx = capi.Context(0)
    dev = [torch.from_numpy(np.ascontiguousarray(w[2].mvImg_Pyr[0])).cuda() for w in ws]
    pin = [torch.from_numpy(np.ascontiguousarray(w[2].mvImg_Pyr[0])).pin_memory() for w in ws]
    torch.cuda.synchronize()
    dptr, pptr = [t.data_ptr() for t in dev], [t.data_ptr() for t in pin]
    if a.only_batch:
        dt = time_batch(ctx, cam, ws, a.only_batch, dptr, a.reps)
        print(f"batch n={a.only_batch} device images: {dt * 1e3:.3f} ms/call, {a.only_batch / dt:.0f} frames/s")
        return
    out = {}
    for n in [int(x) for x in a.n.split(",")]:
        for name, ptrs in (("device", dptr), ("pinned", pptr)):
            dt = time_batch(ctx, cam, ws, n, ptrs, a.reps if n <= 256 else max(3, a.reps // 4))
            out[f"batch_{name}_n{n}"] = dict(ms_per_call=dt * 1e3, frames_per_s=n / dt)
            print(f"dsdtm_track_frames n={n:5d} {name:7s} images: {dt * 1e3:8.3f} ms/call  {n / dt:10.0f} frames/s", flush=True)
    for name, ptrs in (("device", dptr), ("pinned", pptr)):
        rate, per = time_single([ctx], cam, ws, ptrs, 200)
        out[f"single_1ctx_{name}"] = dict(ms_per_call=per * 1e3, frames_per_s=rate)
        print(f"dsdtm_track_frame 1 context / 1 thread, {name} images: {per * 1e3:.3f} ms/call  {rate:.0f} frames/s", flush=True)
    ctxs = [capi.Context(0) for _ in range(a.threads)]
    rate, per = time_single(ctxs, cam, ws, dptr, 100)
    out[f"single_{a.threads}ctx_device"] = dict(frames_per_s=rate)
    print(f"dsdtm_track_frame {a.threads} contexts / {a.threads} threads, device images: {rate:.0f} frames/s", flush=True)
    for c in ctxs:
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
