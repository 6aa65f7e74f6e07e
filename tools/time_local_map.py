"""Times dsdtm_localmap_select (libdsdtm_amd_localmap.so) against select_local_map_host on one CPU thread, and the map's updates.

    python tools/time_local_map.py [--out FILE] [--kernels CSV]          # the table of profiles/r17_local_map.txt
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_local_map.py --trace     # kernel-only times, a run of its own;
                                                                         # its *_kernel_trace.csv is what --kernels folds into the table

Maps: K = 10 / 100 / 1000 / 4000 keyframes of 300 slots along a straight trajectory (a keyframe every 0.5 m, looking sideways at a
wall of points 2-4 m away: 250 points of its own, 50 shared with its predecessor, 5 % of the points bad), so a pose on the trajectory
sees the keyframes within a few metres and no others — a minority of a large map. 64 poses spread over the trajectory. n = 1 / 64 /
1024 descs per call, ALL ON ONE MAP per map size (select only reads it; device memory stays modest). n_local = 10, point_capacity 4096.
Every call is synchronous (it ends in the library's wait), so a host clock around it is the call's time; the descriptors are prepared
once. Each shape is pre-rolled before it is timed; medians and the 10th / 90th percentiles are reported. The answers of the n = 64 call
are held to the host function's bit for bit. The baseline is select_local_map_host (dsdtm_amd/host/dsdtm_localmap_host.hpp) at -O2
-ffp-contract=off on one thread of the same machine in the same run, over the same map and poses, with its scratch kept between
calls: this repository's own straightforward C++, NOT the reference's code.
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsdtm_amd import local_map  # noqa: E402
from tests import local_map_cases as cases  # noqa: E402

SIZES, BATCHES, SLOTS, OWN, N_POSES, N_LOCAL, CAPACITY = (10, 100, 1000, 4000), (1, 64, 1024), 300, 250, 64, 10, 4096
TRACE_CALLS = 5


def trajectory_world(K, seed=17):
    rng = np.random.default_rng(seed)
    x = 0.5 * np.arange(K)
    p = np.stack([np.repeat(x, OWN) + rng.uniform(-1, 1, K * OWN), rng.uniform(-0.7, 0.7, K * OWN), rng.uniform(2, 4, K * OWN)], 1)
    bad = (rng.random(K * OWN) < 0.05).astype(np.uint8)
    slots = []
    for k in range(K):
        prev = rng.integers((k - 1) * OWN, k * OWN, SLOTS - OWN) if k else np.full(SLOTS - OWN, -1)
        slots.append(np.concatenate([np.arange(k * OWN, (k + 1) * OWN), prev]).astype(np.int32))
    T = np.array([cases.pose((-xk, 0.0, 0.0)) for xk in x])
    poses = []
    for c in rng.uniform(0, max(x[-1], 0.5), N_POSES):
        R = np.array(cases.pose(yaw=rng.uniform(-0.1, 0.1))).reshape(3, 4)[:, :3]
        t = -R @ np.array([c, rng.uniform(-0.1, 0.1), rng.uniform(-0.2, 0.2)])
        poses.append(np.hstack([R, t[:, None]]).reshape(12).tolist())
    return dict(name=f"trajectory_{K}", world=dict(p_world=p, bad=bad, T_kf_w=T, slots=slots), poses=poses, n_local=N_LOCAL, boundary=0, capacity=None,
                file_capacity=CAPACITY)


def upload(ctx, w):
    m = ctx.new_map()
    for a in range(0, len(w["p_world"]), 65536):
        m.points_write(a, w["p_world"][a:a + 65536], w["bad"][a:a + 65536])
    for k, s in enumerate(w["slots"]):
        m.keyframe_add(w["T_kf_w"][k], s)
    return m


def _stats(samples):
    s = sorted(samples)
    return dict(median_us=1e6 * statistics.median(s), p10_us=1e6 * s[len(s) // 10], p90_us=1e6 * s[(9 * len(s)) // 10], reps=len(s))


def _timed(fn, reps, preroll):
    for _ in range(preroll):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return _stats(out)


def host_baseline(tmp, cs, reps):
    """select_local_map_host through tests/local_map_host/driver.cpp: ({case: stats}, {case: [answer per pose]})."""
    exe = os.path.join(tmp, "local_map_driver")
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "local_map_host", "driver.cpp")], check=True)
    cases.write_cases(os.path.join(tmp, "cases.bin"), cs)
    out = subprocess.run([exe, os.path.join(tmp, "cases.bin"), "time", str(reps)], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    times, answers = {}, {i: [] for i in range(len(cs))}
    for line in out:
        if line.startswith("time "):
            _, ci, med, p10, p90 = line.split()
            times[int(ci)] = dict(median_us=float(med), p10_us=float(p10), p90_us=float(p90), reps=reps)
            continue
        head, kf, dist, point, point_kf = [part.split() for part in line.split("|")]
        ci, _, n_close, n_kf, n_points, overflow = (int(v) for v in head)
        answers[ci].append(dict(n_close=n_close, n_kf=n_kf, n_points=n_points, overflow=overflow, kf=[int(v) for v in kf], point=[int(v) for v in point],
                                point_kf=[int(v) for v in point_kf], kf_dist=np.array([int(v, 16) for v in dist], np.uint64).view(np.float64).tolist()))
    return times, answers


def fold_kernels(path):
    """Per (K, n) the median kernel time of a select (both launches) from the kernel trace of a --trace run: the selects come in the
    order of SIZES x BATCHES, TRACE_CALLS each."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            if "localmap_visible_kernel" in name or "localmap_select_kernel" in name:
                rows.append((int(r["Start_Timestamp"]), "visible" if "visible" in name else "select", int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    calls, cur = [], None
    for _, kind, ns in rows:           # a call is a visible launch (absent for an empty map: never here) followed by a select launch
        if kind == "visible":
            cur = [ns, 0]
        else:
            cur[1] = ns
            calls.append(cur)
    assert len(calls) == len(SIZES) * len(BATCHES) * TRACE_CALLS, len(calls)
    out, i = {}, 0
    for K in SIZES:
        for n in BATCHES:
            c = calls[i:i + TRACE_CALLS]
            i += TRACE_CALLS
            out[(K, n)] = (statistics.median(v for v, _ in c) / 1e3, statistics.median(s for _, s in c) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", default=None, help="the *_kernel_trace.csv of a --trace run under rocprofv3: adds the kernel times to the table")
    ap.add_argument("--trace", action="store_true", help=f"a short run for rocprofv3 --kernel-trace: {TRACE_CALLS} selects per map size and batch size")
    a = ap.parse_args()
    ctx = local_map.LocalMapContext(0)             # raises without a gfx950 device: this tool measures on the device
    cs = [trajectory_world(K) for K in SIZES]
    if a.trace:
        for c in cs:
            m = upload(ctx, c["world"])
            for n in BATCHES:
                call = local_map.SelectCall(ctx, cases.CAM, [(m, c["poses"][i % N_POSES], CAPACITY) for i in range(n)], N_LOCAL, 0)
                for _ in range(TRACE_CALLS):
                    assert call.run_raw() == 0, ctx.last_error()
            m.close()
        print("trace run done")
        return
    kernels = fold_kernels(a.kernels) if a.kernels else {}
    host_t, host_a = host_baseline(tempfile.mkdtemp(prefix="local_map_host_"), cs, 20)
    lines = [f"{'row':<52} {'median us':>11} {'p10':>10} {'p90':>10} {'per select':>11} {'x host':>8} {'kernels us (visible + select)':>30}"]
    rows, updates = {}, {}
    for ci, c in enumerate(cs):
        K = len(c["world"]["slots"])
        m = upload(ctx, c["world"])
        h = host_t[ci]
        rows[f"host K = {K}"] = h
        close = statistics.mean(r["n_close"] for r in host_a[ci])
        pts = statistics.mean(r["n_points"] for r in host_a[ci])
        lines.append(f"{'select_local_map_host, one thread, K = %d' % K:<52} {h['median_us']:>11.1f} {h['p10_us']:>10.1f} {h['p90_us']:>10.1f} {h['median_us']:>11.2f} {1.0:>8.2f}"
                     f"   (mean {close:.1f} close keyframes, {pts:.0f} local points)")
        for n in BATCHES:
            call = local_map.SelectCall(ctx, cases.CAM, [(m, c["poses"][i % N_POSES], CAPACITY) for i in range(n)], N_LOCAL, 0)

            def run():
                assert call.run_raw() == 0, ctx.last_error()
            r = _timed(run, {1: 200, 64: 50, 1024: 10}[n], 5)
            r["per_select_us"] = r["median_us"] / n
            rows[f"device K = {K} n = {n}"] = r
            if n == N_POSES:                       # the timed answers are the host function's, bit for bit
                for q, got in enumerate(call.answers()):
                    cases.same_answer(got, host_a[ci][q], (K, q))
            kt = kernels.get((K, n))
            lines.append(f"{'dsdtm_localmap_select K = %d, n = %d' % (K, n):<52} {r['median_us']:>11.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f} {r['per_select_us']:>11.2f} "
                         f"{h['median_us'] / r['per_select_us']:>8.2f} " + (f"{kt[0]:>14.1f} + {kt[1]:.1f}" if kt else f"{'-':>30}"))
        if K == 1000:                              # the updates: the call returns at once; with the wait = 200 calls and one select, per call
            rng = np.random.default_rng(3)
            P = len(c["world"]["p_world"])
            slots, T = rng.integers(-1, P, SLOTS).astype(np.int32), np.array(cases.pose((1.0, 0, 0)))
            X = rng.uniform(-1, 1, (300, 3)) + [0, 0, 3]
            wait = local_map.SelectCall(ctx, cases.CAM, [(m, c["poses"][0], CAPACITY)], N_LOCAL, 0)
            for name, fn in (("dsdtm_localmap_keyframe_add (300 slots)", lambda: m.keyframe_add(T, slots)),
                             ("dsdtm_localmap_points_write (300 points, rewrite)", lambda: m.points_write(1000, X))):
                r = _timed(fn, 200, 10)
                wait.run_raw()
                t0 = time.perf_counter()
                for _ in range(200):
                    fn()
                wait.run_raw()
                r["with_wait_us"] = 1e6 * (time.perf_counter() - t0) / 200
                updates[name] = r
        m.close()
    for name, r in updates.items():
        lines.append(f"{name + ', K = 1000':<52} {r['median_us']:>11.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f}   (through the Python binding; 200 calls and one select's wait: "
                     f"{r['with_wait_us']:.1f} us per call)")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(tool="time_local_map", maps_per_size=1, rows=rows, updates=updates)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
