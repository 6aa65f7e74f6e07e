"""Tracked frames per second through dsdtm_track_frames (one call = n frames of n independent trackers) against dsdtm_track_frame
(one call per frame: 1 context on 1 thread, and 16 contexts on 16 threads).

    python tools/track_batch_rate.py [--n 1,16,64,256,1024] [--reps 20] [--threads 16] [--only-batch N]
    python tools/track_batch_rate.py --resident [--n 16,64,256] [--reps 20] [--rounds 5]
    python tools/track_batch_rate.py --images-only [--n 16,64,256] [--reps 20]

World: 640x480, 300 reference features and 900 map points per frame (8 distinct worlds, repeated). Images either in device
memory (a torch tensor per frame) or in pinned host memory. Prints one line per configuration and a JSON summary at the end.
`--only-batch N` runs just the device-image batch of N frames (for a rocprofv3 --kernel-trace --stats run of the stages; with
`--resident`: the resident loop of N frames).
`--resident`: the lockstep loop on resident frames against the call on images, ALTERNATING in one process, `--rounds` times
each: per step, dsdtm_frame_prefetch of step k + 1 for every tracker (n calls), then dsdtm_track_frames on step k's frames
(image == NULL: the call starts at Run), then step k's frames destroyed — wall per step, the n prefetch calls and n destroys
included; beside it the host time of the n prefetch calls alone. Median and spread (min..max) over the rounds.
`--images-only`: the image batch alone, one line per n and memory (for A/B runs of two libraries, one process each)."""
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


def time_resident(ctx, cam, ws, n, ptrs, reps):
    """(wall per lockstep step, host time of the n prefetch calls of a step) on resident frames."""
    import ctypes as C
    call = tracking.TrackBatchCall(ctx, cam, frames_of(ws, n, [w[2].mvImg_Pyr[0] for w in ws]))
    lib = ctx.lib
    ims = []
    for f in range(n):
        im = capi.FrameImage()
        im.gray, im.width, im.height, im.stride, im.levels = ptrs[f % len(ptrs)], cam.width, cam.height, cam.width, 5
        ims.append(im)
        call.descs[f].image = None
    hnd = C.c_void_p()
    t_pref = [0.0]

    def prefetch():
        t0 = time.perf_counter()
        out = []
        for f in range(n):
            ctx.check(lib.dsdtm_frame_prefetch(ctx.handle, C.byref(ims[f]), C.byref(hnd)))
            out.append(hnd.value)
        t_pref[0] += time.perf_counter() - t0
        return out

    def loop(m):
        nxt = prefetch()
        for _ in range(m):
            cur, nxt = nxt, prefetch()
            for f in range(n):
                call.res[f].frame = cur[f]
            ctx.check(lib.dsdtm_track_frames(ctx.handle, C.byref(call.cs), n, call.descs, call.res, call.matches.ctypes.data,
                                             call.rn.ctypes.data, call.in_grid.ctypes.data))
            for h in cur:
                lib.dsdtm_frame_destroy(ctx.handle, h)
        for h in nxt:
            lib.dsdtm_frame_destroy(ctx.handle, h)
    loop(3)
    t_pref[0] = 0.0
    t0 = time.perf_counter()
    loop(reps)
    dt = (time.perf_counter() - t0) / reps
    return dt, t_pref[0] / (reps + 1)


def resident_report(ctx, cam, ws, ns, mem, reps, rounds):
    out = {}
    for n in ns:
        for name, ptrs in mem:
            img, res, pre = [], [], []
            for _ in range(rounds):                                   # the two paths alternate
                img.append(time_batch(ctx, cam, ws, n, ptrs, reps))
                r, p = time_resident(ctx, cam, ws, n, ptrs, reps)
                res.append(r); pre.append(p)
            med = lambda v: float(np.median(v))
            out[f"n{n}_{name}"] = dict(image_ms=med(img) * 1e3, image_ms_range=[min(img) * 1e3, max(img) * 1e3], resident_ms=med(res) * 1e3,
                                       resident_ms_range=[min(res) * 1e3, max(res) * 1e3], prefetch_calls_ms=med(pre) * 1e3,
                                       image_frames_per_s=n / med(img), resident_frames_per_s=n / med(res))
            print(f"n={n:4d} {name:7s}: images {med(img) * 1e3:7.3f} ms/call ({min(img) * 1e3:.3f}..{max(img) * 1e3:.3f}) {n / med(img):8.0f} frames/s | "
                  f"resident {med(res) * 1e3:7.3f} ms/step ({min(res) * 1e3:.3f}..{max(res) * 1e3:.3f}) {n / med(res):8.0f} frames/s, "
                  f"of it the {n} prefetch calls on the host {med(pre) * 1e3:.3f} ms", flush=True)
    print(json.dumps(out))


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
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--images-only", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    ws = worlds()
    cam = ws[0][0]
    ctx = capi.Context(0)
    dev = [torch.from_numpy(np.ascontiguousarray(w[2].mvImg_Pyr[0])).cuda() for w in ws]
    pin = [torch.from_numpy(np.ascontiguousarray(w[2].mvImg_Pyr[0])).pin_memory() for w in ws]
    torch.cuda.synchronize()
    dptr, pptr = [t.data_ptr() for t in dev], [t.data_ptr() for t in pin]
    if a.only_batch and a.resident:
        dt, pre = time_resident(ctx, cam, ws, a.only_batch, dptr, a.reps)
        print(f"resident n={a.only_batch} device images: {dt * 1e3:.3f} ms/step, {a.only_batch / dt:.0f} frames/s")
        return
    if a.resident or a.images_only:
        ns = [int(x) for x in (a.n if a.n != "1,16,64,256,1024" else "16,64,256").split(",")]
        mem = (("device", dptr), ("pinned", pptr))
        if a.resident:
            resident_report(ctx, cam, ws, ns, mem, a.reps, a.rounds)
        else:
            for n in ns:
                for name, ptrs in mem:
                    dt = time_batch(ctx, cam, ws, n, ptrs, a.reps)
                    print(f"images n={n:4d} {name:7s}: {dt * 1e3:8.3f} ms/call", flush=True)
        return
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
