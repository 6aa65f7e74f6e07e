"""Times dsdtm_slam_track_commit and dsdtm_slam_need_keyframes (libdsdtm_amd_slam.so) against their baselines.

    python tools/time_aftertrack.py [--out FILE]          # the table of profiles/r21_aftertrack.txt

Maps: those of tools/time_track_map.py (K = 10 / 100 / 1000 / 4000 keyframes of 300 slots along a straight trajectory), n = 1 / 64 / 1024
frames per call, all on ONE map (the shape of a rig; the walk of one map's descs is serial on the device, so this is the entry's slowest
shape per frame). A frame has 200 matches. Every call is synchronous, so a host clock around it is the call's time; descriptors are
prepared once; each shape is pre-rolled; medians and the 10th / 90th percentiles are reported.
COMMIT. `no bad`: every norm below the threshold (the found counts grow, the cascade's blocks return at once: the call is repeatable).
`one bad`: n = 1, the first match is a fresh point with found count 0 and a norm above the threshold in every repetition, so the
cascade streams the slot pool. Baselines: track_commit_host on one thread (tools/aftertrack_host_timer.cpp, -O2 -ffp-contract=off, the
same shapes), and THE PATH WITHOUT THE ENTRY: that host function's time plus found_write of the 200 counts (+ points_write of the bad
point and one keyframe_write per touched keyframe for `one bad`), host time until the calls have RETURNED — they are asynchronous, so
this favours the baseline: the device's work is not waited for.
NEED-KEYFRAMES. 200 current points, the newest keyframe (300 slots), 10 local keyframes. Baselines: gather_keyframe_desc_host on one
thread (the gather alone; need_keyframe_host's own time is in profiles/r13_need_keyframe.txt and is not measured again here), and
dsdtm_need_keyframes on the host-gathered arrays of the same trackers (arrays prepared once: the call alone, without the gather).
Kernel-only times need a profiler run of their own and are not part of this table.
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsdtm_amd import aftertrack_restatement as AR  # noqa: E402
from dsdtm_amd import capi, slam  # noqa: E402
from dsdtm_amd.keyframe_decision import KeyframeParams  # noqa: E402
from tools.time_local_map import BATCHES, SIZES  # noqa: E402
from tools.time_track_map import timed, track_world, upload  # noqa: E402

MATCHES, CUR, LOCAL_KF, THR = 200, 200, 10, 1.0
CAM = capi.camera_struct(type("Cam", (), dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0, f=512.0, width=640, height=480))())


def host_times(tmp, w, match, victims, cur, kf, lk):
    exe = os.path.join(tmp, "aftertrack_host_timer")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "aftertrack_host_timer.cpp")], check=True)
    path = os.path.join(tmp, "world.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("2i", len(w["p_world"]), len(w["slots"])))
        f.write(np.ascontiguousarray(w["p_world"], np.float64).tobytes() + np.ascontiguousarray(w["bad"], np.uint8).tobytes())
        f.write(np.ascontiguousarray(w["found"], np.int32).tobytes() + np.ascontiguousarray(w["T_kf_w"], np.float64).tobytes())
        f.write(np.array([len(s) for s in w["slots"]], np.int32).tobytes())
        for key, dt in (("slots", np.int32), ("observes", np.uint8)):
            for a in w[key]:
                f.write(np.ascontiguousarray(a, dt).tobytes())
        f.write(struct.pack("5i", len(match), len(victims), len(cur), kf, len(lk)))
        for a in (match, victims, cur, lk):
            f.write(np.asarray(a, np.int32).tobytes())
    out = {}
    for line in subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.strip().split("\n"):
        v = line.split()
        out[v[0]] = dict(median_us=float(v[1]), p10_us=float(v[2]), p90_us=float(v[3]), reps=len(victims))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = slam.SlamContext(0)                       # raises without a gfx950 device: this tool measures on the device
    kctx = capi.KeyframeContext(0)
    lines = [f"{'row':<74} {'median us':>11} {'p10':>10} {'p90':>10} {'per item':>10} {'x host':>8}"]
    rows = {}

    def row(name, r, n=1, host=None):
        r["per_item_us"] = r["median_us"] / n
        rows[name] = r
        lines.append(f"{name:<74} {r['median_us']:>11.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f} {r['per_item_us']:>10.2f} "
                     + (f"{host['median_us'] / r['per_item_us']:>8.2f}" if host else f"{'':>8}"))
    with tempfile.TemporaryDirectory(prefix="aftertrack_host_") as tmp:
        for K in SIZES:
            w = track_world(K)["world"]
            P, kf = len(w["p_world"]), K - 1
            rng = np.random.default_rng(21 + K)
            good = np.flatnonzero(np.asarray(w["bad"]) == 0)
            match = rng.choice(good, MATCHES, replace=False).astype(np.int32)
            reps = 30 if K >= 1000 else 60
            observed = np.unique(np.concatenate([np.asarray(s)[np.asarray(o) != 0] for s, o in zip(w["slots"], w["observes"])]))
            pool = np.setdiff1d(np.intersect1d(observed, good), match)
            victims = rng.choice(pool, 2 * reps + 4, replace=False).astype(np.int32)      # host timer: the first `reps`; device: the rest
            cur = rng.choice(good, CUR, replace=False).astype(np.int32)
            lk = list(range(max(0, K - 1 - LOCAL_KF), K - 1))[:LOCAL_KF] or [0]
            host = host_times(tmp, w, match, victims[:reps], cur, kf, lk)
            lines.append(f"--- K = {K}: {P} points, {sum(len(s) for s in w['slots'])} slots; {MATCHES} matches per frame; {CUR} current points, {len(lk)} local keyframes")
            for name in ("track_commit_host_no_bad", "track_commit_host_one_bad", "gather_keyframe_desc_host"):
                row(f"{name}, one thread, K = {K}", host[name])
            m = upload(ctx, w)
            low = np.zeros(MATCHES)
            for n in BATCHES:
                call = slam.CommitCall(ctx, THR, [(m, match, low)] * n, 8, want_found_after=False)

                def run():
                    assert call.run_raw() == 0, ctx.last_error()
                row(f"dsdtm_slam_track_commit no bad K = {K}, n = {n}", timed(run, {1: 100, 64: 20, 1024: 5}[n], 2), n, host["track_commit_host_no_bad"])
            # one point goes bad per call: a fresh victim each time
            vic = list(victims[reps:])
            m.found_write(vic, np.zeros(len(vic), np.int32))
            high = low.copy()
            high[0] = 2.0
            calls = [slam.CommitCall(ctx, THR, [(m, np.concatenate([[v], match[1:]]).astype(np.int32), high)], 8, want_found_after=False) for v in vic]
            it = iter(calls)

            def one_bad():
                c = next(it)
                assert c.run_raw() == 0 and c.results[0].n_bad == 1, ctx.last_error()
            row(f"dsdtm_slam_track_commit one bad K = {K}, n = 1", timed(one_bad, reps, 2), 1, host["track_commit_host_one_bad"])
            # the path without the entry: the host function, then the writes (until they have returned)
            counts = np.arange(MATCHES, dtype=np.int32)

            def writes_no_bad():
                m.found_write(match, counts)
            r = timed(writes_no_bad, 100, 2)
            r["median_us"] += host["track_commit_host_no_bad"]["median_us"]
            row(f"without the entry, no bad: host function + found_write K = {K}", r)
            world_now = m.read()
            p = int(vic[-1])
            touched = [k for k, s in enumerate(world_now["slots"]) if (np.asarray(s) == p).any()] or [0]

            def writes_one_bad():
                m.found_write(match, counts)
                m.points_write(p, [world_now["p_world"][p]], [1], [0])
                for k in touched:
                    m.keyframe_write(k, None, 0, world_now["slots"][k], world_now["observes"][k])
            r = timed(writes_one_bad, 50, 2)
            r["median_us"] += host["track_commit_host_one_bad"]["median_us"]
            row(f"without the entry, one bad: + points_write + {len(touched)} keyframe_write K = {K}", r)
            # need-keyframes
            T = np.asarray(w["T_kf_w"][kf], np.float64).reshape(12).copy()
            T[3] += 0.05
            tracker = dict(map=m, T_cur_w=T, n_valid=CUR, cur_point=cur, kf=kf, local_kf=lk)
            g = AR.gather_keyframe_desc(world_now, T, CUR, cur, kf, lk)
            for n in BATCHES:
                call = slam.KeyframeCall(ctx, CAM, KeyframeParams(), [tracker] * n)

                def run_kf():
                    assert call.run_raw() == 0, ctx.last_error()
                row(f"dsdtm_slam_need_keyframes K = {K}, n = {n}", timed(run_kf, {1: 100, 64: 20, 1024: 5}[n], 2), n, host["gather_keyframe_desc_host"])
                old = capi.KeyframeCall(kctx, CAM, KeyframeParams(), [g] * n)

                def run_old():
                    assert old.run_raw() == 0
                row(f"dsdtm_need_keyframes on host-gathered arrays (the call alone) K = {K}, n = {n}", timed(run_old, {1: 100, 64: 20, 1024: 5}[n], 2), n)
            m.close()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(tool="time_aftertrack", rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    t0 = time.perf_counter()
    main()
    print(f"# {time.perf_counter() - t0:.0f} s", file=sys.stderr)
