"""Times dsdtm_mapping_covisibility, dsdtm_mapping_ba_window and dsdtm_mapping_ba_commit (libdsdtm_amd_mapping.so) against
update_connection_host, ba_window_host and ba_commit_host on one CPU thread, and one whole mapping step on the device against today's path.

    python tools/time_ba_window.py [--out FILE]          # the table of profiles/r19_ba_window.txt

Maps: those of tools/time_track_map.py (K = 10 / 100 / 1000 / 4000 keyframes of 300 slots along a straight trajectory). The window is the
newest keyframe's, with the strongest 15 entries of its covisibility list (so that at most 16 keyframes are free). n = 1 / 16 / 256 pairs
or windows per call, all the SAME keyframe of one map: that is what the entries cost per window, but windows of one keyframe overlap,
so the commit is timed at n = 1 only (no observation flagged and the window's own poses and points: the call is repeatable). Every call
is synchronous, so a host clock around it is the call's time; descriptors and device arrays are prepared once; each shape is pre-rolled;
medians and the 10th / 90th percentiles are reported. The host functions run at -O2 -ffp-contract=off on one thread of the same
machine in the same run over the same flat arrays (tools/ba_window_host_timer.cpp): this repository's own straightforward C++, NOT the
reference's walk over std::map<KeyFrame*, ...> per MapPoint. THE STEP: Optimizer.LocalBundleAdjustmentOnDevice (window + dsdtm_local_ba_batch_device +
commit, the allocation of its device arrays included) on a freshly uploaded map, once after one warm-up on another fresh map, against
ba_window_host + dsdtm_local_ba on host arrays + dsdtm_mapping_points_write / _keyframe_write of the results (points in runs of
consecutive indices). The worlds' bearings are random, so the solve is not a realistic one; it is the same problem on both sides.
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

from dsdtm_amd import ba_window, capi  # noqa: E402
from dsdtm_amd.optimizer import Optimizer, local_bundle_adjustment  # noqa: E402
from tools.time_local_map import SIZES  # noqa: E402
from tools.time_track_map import timed, track_world, upload  # noqa: E402

BATCHES = (1, 16, 256)
DELTA = 2.0 / 500.0


def host_times(tmp, w, kf, cov, reps):
    exe = os.path.join(tmp, "ba_window_host_timer")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "ba_window_host_timer.cpp")], check=True)
    path = os.path.join(tmp, "world.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("2i", len(w["p_world"]), len(w["slots"])))
        f.write(np.ascontiguousarray(w["p_world"], np.float64).tobytes() + np.ascontiguousarray(w["bad"], np.uint8).tobytes())
        f.write(np.ascontiguousarray(w["found"], np.int32).tobytes() + np.ascontiguousarray(w["T_kf_w"], np.float64).tobytes())
        f.write(np.array([len(s) for s in w["slots"]], np.int32).tobytes())
        for key, dt in (("slots", np.int32), ("observes", np.uint8), ("px", np.float32), ("level", np.int32), ("bearing", np.float64)):
            for a in w[key]:
                f.write(np.ascontiguousarray(a, dt).tobytes())
        f.write(struct.pack("3i", kf, -1, len(cov)) + np.array(cov, np.int32).tobytes() + struct.pack("i", reps))
    out, counts = {}, None
    for line in subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.strip().split("\n"):
        v = line.split()
        if v[0] == "window":
            counts = dict(zip(("n_local", "n_fixed", "n_points", "n_obs", "usable"), (int(x) for x in v[1:6])))
        else:
            out[v[0]] = dict(median_us=float(v[1]), p10_us=float(v[2]), p90_us=float(v[3]), reps=reps)
    return out, counts


def host_step(mctx, ctx, w, win, host_window_us):
    """Today's path: the set construction on the host, dsdtm_local_ba on host arrays, the results written into the resident map."""
    m = upload(mctx, w)
    T, X = win["T_c2w"].reshape(-1).copy(), win["points"].reshape(-1).copy()
    t0 = time.perf_counter()
    local_bundle_adjustment(ctx, T, win["kf_constant"], X, win["obs_kf"], win["obs_point"], win["obs_bearing"], win["obs_level"], DELTA)
    t1 = time.perf_counter()
    for i, k in enumerate(win["kf_index"]):
        m.keyframe_write(int(k), T.reshape(-1, 12)[i])
    order = np.argsort(win["point_index"])
    idx, Xs = win["point_index"][order], X.reshape(-1, 3)[order]
    starts = np.flatnonzero(np.diff(idx, prepend=idx[0] - 2) != 1) if len(idx) else []
    for a, b in zip(starts, list(starts[1:]) + [len(idx)]):
        m.points_write(int(idx[a]), Xs[a:b])
    m.read()                                                    # (the updates are asynchronous: wait for them)
    t2 = time.perf_counter()
    m.close()
    return dict(window_us=host_window_us, solve_us=1e6 * (t1 - t0), write_us=1e6 * (t2 - t1), total_us=host_window_us + 1e6 * (t2 - t0), write_calls=len(win["kf_index"]) + len(starts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    mctx = ba_window.MappingContext(0)             # raises without a gfx950 device: this tool measures on the device
    ctx = capi.default_context(0, diag=False)
    lines = [f"{'row':<66} {'median us':>11} {'p10':>10} {'p90':>10} {'per item':>10} {'x host':>8}"]
    rows = {}

    def row(name, r, n=1, host=None):
        r["per_item_us"] = r["median_us"] / n
        rows[name] = r
        lines.append(f"{name:<66} {r['median_us']:>11.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f} {r['per_item_us']:>10.2f} "
                     + (f"{host['median_us'] / r['per_item_us']:>8.2f}" if host else f"{'':>8}"))
    with tempfile.TemporaryDirectory(prefix="ba_window_host_") as tmp:
        for K in SIZES:
            w = track_world(K)["world"]
            kf = K - 1
            m = upload(mctx, w)
            full = mctx.covisibility([(m, kf, 4096)])[0]
            cov = full["cov_kf"][-15:]
            host, counts = host_times(tmp, w, kf, cov, 20 if K >= 1000 else 100)
            lines.append(f"--- K = {K}: covisibility list {full['n_cov']} of {full['n_connected']} connected; window {counts}")
            for name in ("update_connection_host", "ba_window_host", "ba_commit_host"):
                if name in host:
                    row(f"{name}, one thread, K = {K}", host[name])
            pcap, ocap = counts["n_points"] + 64, counts["n_obs"] + 256
            for n in BATCHES:
                reps = {1: 100, 16: 20, 256: 5}[n]
                pairs = [(m, kf, 256)] * n
                row(f"dsdtm_mapping_covisibility K = {K}, n = {n}", timed(lambda: mctx.covisibility(pairs), reps, 2), n, host["update_connection_host"])
                call = ba_window.WindowCall(mctx, [(m, kf, cov, -1, 80, pcap, ocap)] * n)

                def run():
                    assert call.run_raw() == 0, mctx.last_error()
                row(f"dsdtm_mapping_ba_window K = {K}, n = {n}", timed(run, reps, 2), n, host["ba_window_host"])
                if n == 1 and counts["usable"]:
                    win = call.answers()[0]
                    assert win["usable"] and (win["n_points"], win["n_obs"]) == (counts["n_points"], counts["n_obs"])
                    flags = torch.zeros(ocap, dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()

                    def commit():
                        st, _ = call.commit(flags, None, 8)
                        assert st == 0, mctx.last_error()
                    row(f"dsdtm_mapping_ba_commit K = {K}, n = 1", timed(commit, reps, 2), 1, host.get("ba_commit_host"))
                del call
            m.close()
            if counts["usable"]:
                dev = []
                for _ in range(2):                                  # (the first one warms up)
                    m = upload(mctx, w)
                    t0 = time.perf_counter()
                    got = Optimizer.LocalBundleAdjustmentOnDevice(mctx, m, kf, cov, -1, DELTA, ctx=ctx, capacities=(80, pcap, ocap))
                    dev.append(1e6 * (time.perf_counter() - t0))
                    m.close()
                hs = host_step(mctx, ctx, w, got["window"], host["ba_window_host"]["median_us"])
                rows[f"step K = {K}"] = dict(device_us=dev[1], host=hs, iterations=got["summary"]["iterations"])
                lines.append(f"{'mapping step on the device (window + solve + commit) K = %d' % K:<66} {dev[1]:>11.1f}   ({got['summary']['iterations']} iterations, "
                             f"{got['commit']['n_outliers']} outliers, {got['commit']['n_bad']} points went bad)")
                lines.append(f"{'mapping step, today (host window + dsdtm_local_ba + writes) K = %d' % K:<66} {hs['total_us']:>11.1f}   (window {hs['window_us']:.1f}, "
                             f"solve {hs['solve_us']:.1f}, {hs['write_calls']} write calls {hs['write_us']:.1f})")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(tool="time_ba_window", rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
