"""Times dsdtm_trackmap_local (libdsdtm_amd_trackmap.so) against select_local_map_host + flatten_local_map_host on one CPU thread.

    python tools/time_track_map.py [--out FILE]          # the table of profiles/r18_track_map.txt

Maps: those of tools/time_local_map.py (K = 10 / 100 / 1000 / 4000 keyframes of 300 slots along a straight trajectory, n_local 10, about
2400 local points), each point observed by the keyframes that list it (a point listed twice by one keyframe is observed by the first
of the two slots), random pixel / level / bearing columns and found counts. n = 1 / 64 / 1024 descs per call, all on one map per map
size. Two capacity settings per shape, because the read-back is sized by the capacities: `fit` (point_capacity and obs_capacity the
largest need among the poses) and `roomy` (4096 points, 8192 observations). Every call is synchronous, so a host clock around it is the
call's time; the descriptors are prepared once; each shape is pre-rolled; medians and the 10th / 90th percentiles are reported. The
answers of the n = 64 call are held to the host functions' bit for bit. The baseline is select_local_map_host + flatten_local_map_host
(dsdtm_amd/host) at -O2 -ffp-contract=off on one thread of the same machine in the same run over the same flat arrays, scratch kept
between calls: this repository's own straightforward C++, NOT the reference's walk over std::map<KeyFrame*, ...> per MapPoint, which
chases pointers and would be slower. Kernel-only times need a profiler run of their own and are not part of this table.
"""
import argparse
import json
import os
import subprocess
import sys
import statistics
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsdtm_amd import track_map  # noqa: E402
from tests import track_map_cases as cases  # noqa: E402
from tools.time_local_map import BATCHES, N_LOCAL, N_POSES, SIZES, trajectory_world  # noqa: E402  (the issue's maps: the same worlds as r17)

ROOMY = (4096, 8192)


def timed(fn, reps, preroll):
    for _ in range(preroll):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    out.sort()
    return dict(median_us=1e6 * statistics.median(out), p10_us=1e6 * out[len(out) // 10], p90_us=1e6 * out[(9 * len(out)) // 10], reps=len(out))


def track_world(K):
    c = trajectory_world(K)
    w, rng = c["world"], np.random.default_rng(18 + K)
    w["found"] = rng.integers(0, 100, len(w["p_world"])).astype(np.int32)
    w["observes"], w["px"], w["level"], w["bearing"] = [], [], [], []
    for s in w["slots"]:
        first = np.zeros(len(s), np.uint8)
        first[np.unique(s, return_index=True)[1]] = 1
        w["observes"].append(first * (s >= 0).astype(np.uint8))
        w["px"].append(rng.uniform(0, 480, (len(s), 2)).astype(np.float32))
        w["level"].append(rng.integers(0, 4, len(s)).astype(np.int32))
        w["bearing"].append(rng.normal(size=(len(s), 3)))
    c.update(point_capacity=ROOMY[0], obs_capacity=None, file_obs_capacity=ROOMY[1])
    return c


def upload(ctx, w):
    m = ctx.new_map()
    for a in range(0, len(w["p_world"]), 65536):
        m.points_write(a, w["p_world"][a:a + 65536], w["bad"][a:a + 65536], w["found"][a:a + 65536])
    for k, s in enumerate(w["slots"]):
        m.keyframe_add(w["T_kf_w"][k], s, w["observes"][k], w["px"][k], w["level"][k], w["bearing"][k])
    return m


def host_baseline(tmp, cs, reps):
    exe = os.path.join(tmp, "track_map_driver")
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "track_map_host", "driver.cpp")], check=True)
    cases.write_cases(os.path.join(tmp, "cases.bin"), cs)
    out = subprocess.run([exe, os.path.join(tmp, "cases.bin"), os.path.join(tmp, "answers.bin"), str(reps)], capture_output=True, text=True, check=True).stdout
    times = {}
    for line in out.strip().split("\n"):
        _, ci, med, p10, p90, sel = line.split()
        times[int(ci)] = dict(median_us=float(med), p10_us=float(p10), p90_us=float(p90), select_median_us=float(sel), reps=reps)
    return times, cases.read_answers(os.path.join(tmp, "answers.bin"), cs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = track_map.TrackMapContext(0)             # raises without a gfx950 device: this tool measures on the device
    cs = [track_world(K) for K in SIZES]
    with tempfile.TemporaryDirectory(prefix="track_map_host_") as tmp:      # (the driver, its cases and its answers: gone afterwards)
        host_t, host_a = host_baseline(tmp, cs, 10)
    lines = [f"{'row':<58} {'median us':>11} {'p10':>10} {'p90':>10} {'per desc':>10} {'x host':>8} {'read-back B/desc':>17}"]
    rows = {}
    for ci, c in enumerate(cs):
        K = len(c["world"]["slots"])
        m = upload(ctx, c["world"])
        h, ans = host_t[ci], host_a[ci]
        pts, obs = max(r["n_points"] for r in ans), max(r["n_obs"] for r in ans)
        rows[f"host K = {K}"] = h
        lines.append(f"{'host select + flatten, one thread, K = %d' % K:<58} {h['median_us']:>11.1f} {h['p10_us']:>10.1f} {h['p90_us']:>10.1f} {h['median_us']:>10.2f} {1.0:>8.2f}"
                     f"   (select alone {h['select_median_us']:.1f}; at most {pts} local points, {obs} observations: {33 * pts + 40 * obs} B used)")
        for n in BATCHES:
            for name, (cap, ocap) in (("fit", (pts, obs)), ("roomy", ROOMY)):
                call = track_map.LocalCall(ctx, cases.CAM, [(m, c["poses"][i % N_POSES], cap, ocap) for i in range(n)], N_LOCAL, 0)

                def run():
                    assert call.run_raw() == 0, ctx.last_error()
                r = timed(run, {1: 200, 64: 30, 1024: 5}[n], 3)
                r["per_desc_us"], r["readback_bytes_per_desc"] = r["median_us"] / n, 45 * cap + 4 + 40 * ocap + 8 * N_LOCAL + 4 * N_LOCAL + 32
                rows[f"device K = {K} n = {n} {name}"] = r
                if n == N_POSES and name == "roomy":       # the timed answers are the host functions', bit for bit
                    for q, got in enumerate(call.answers()):
                        cases.same_answer(got, ans[q], (K, q))
                lines.append(f"{'dsdtm_trackmap_local K = %d, n = %d, %s' % (K, n, name):<58} {r['median_us']:>11.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f} "
                             f"{r['per_desc_us']:>10.2f} {h['median_us'] / r['per_desc_us']:>8.2f} {r['readback_bytes_per_desc']:>17d}")
                del call
        m.close()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(tool="time_track_map", maps_per_size=1, rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
