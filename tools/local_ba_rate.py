"""Local bundle adjustment rate: dsdtm_local_ba (one problem from host arrays, copies included) and
dsdtm_local_ba_batch_device (n independent problems in one launch, device arrays).

    python tools/local_ba_rate.py [--n 1,16,64,256] [--reps 10] [--only-batch N]

Problem: a representative DSDTM window — 10 free keyframes, 20 fixed, 3000 points, ~10 000 observations, 10 iterations
(tests/local_ba_restatement.make_world). Device time from HIP events around the launch; wall time of the host entry from
time.perf_counter. Prints one line per configuration and a JSON summary. `--only-batch N` runs just one batch of N (for a
rocprofv3 --kernel-trace --stats run)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dsdtm_amd import capi  # noqa: E402
from dsdtm_amd.optimizer import local_bundle_adjustment  # noqa: E402
from tests import local_ba_restatement as R  # noqa: E402


def problem(seed=100):
    return R.make_world(seed, n_free=10, n_fixed=20, n_points=3000, max_obs=4)


def pack(ws):
    dev = torch.device("cuda:0")
    probs = (capi.LocalBaProblem * len(ws))()
    ko = po = oo = 0
    for j, w in enumerate(ws):
        probs[j] = capi.LocalBaProblem(len(w.T), len(w.points), len(w.obs_kf), 0, ko, po, oo)
        ko += len(w.T); po += len(w.points); oo += len(w.obs_kf)
    cat = lambda xs, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(xs), dt)).to(dev)
    a = dict(T=cat([w.T.reshape(-1) for w in ws], np.float64), kc=cat([w.constant for w in ws], np.uint8),
             X=cat([w.points.reshape(-1) for w in ws], np.float64), okf=cat([w.obs_kf for w in ws], np.int32),
             opt=cat([w.obs_pt for w in ws], np.int32), b=cat([w.bearing.reshape(-1) for w in ws], np.float64),
             lev=cat([w.level for w in ws], np.int32))
    a["out"] = torch.zeros(max(oo, 1), dtype=torch.uint8, device=dev)
    a["sm"] = torch.zeros(len(ws) * capi.LBA_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    return probs, a


def launch(ctx, probs, a, delta, stream):
    f = ctx.lib.dsdtm_local_ba_batch_device
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 7 + [C.POINTER(capi.LocalBaParams), C.c_void_p, C.c_void_p, C.c_void_p]
    prm = capi.LocalBaParams(10, 0, delta)
    ctx.check(f(ctx.handle, len(probs), C.cast(probs, C.c_void_p), a["T"].data_ptr(), a["kc"].data_ptr(), a["X"].data_ptr(),
                a["okf"].data_ptr(), a["opt"].data_ptr(), a["b"].data_ptr(), a["lev"].data_ptr(), C.byref(prm),
                a["out"].data_ptr(), a["sm"].data_ptr(), C.c_void_p(stream.cuda_stream)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,16,64,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-batch", type=int, default=0)
    args = ap.parse_args()
    ctx = capi.default_context(0)
    w = problem()
    print(f"problem: {int((~w.constant).sum())} free + {int(w.constant.sum())} fixed keyframes, {len(w.points)} points, "
          f"{len(w.obs_kf)} observations", flush=True)
    stream = torch.cuda.current_stream()
    if args.only_batch:
        probs, a = pack([w] * args.only_batch)
        launch(ctx, probs, a, w.delta, stream)
        stream.synchronize()
        return
    res = {}
    # the host entry: copies + launch + copies back, wall time
    for _ in range(2):
        T, X = w.T.reshape(-1).copy(), w.points.reshape(-1).copy()
        local_bundle_adjustment(ctx, T, w.constant, X, w.obs_kf, w.obs_pt, w.bearing, w.level, w.delta)
    wall = []
    for _ in range(args.reps):
        T, X = w.T.reshape(-1).copy(), w.points.reshape(-1).copy()
        t0 = time.perf_counter()
        _, sm = local_bundle_adjustment(ctx, T, w.constant, X, w.obs_kf, w.obs_pt, w.bearing, w.level, w.delta)
        wall.append(time.perf_counter() - t0)
    res["host_entry_wall_ms"] = 1e3 * float(np.median(wall))
    res["summary"] = {k: (v if isinstance(v, int) else float(v)) for k, v in sm.items()}
    print(f"dsdtm_local_ba (host arrays, copies included): median {res['host_entry_wall_ms']:.3f} ms wall "
          f"({sm['iterations']} iterations, {sm['successful_steps']} successful)", flush=True)
    for n in [int(v) for v in args.n.split(",")]:
        probs, a = pack([w] * n)
        launch(ctx, probs, a, w.delta, stream)          # warm-up (workspace allocation)
        stream.synchronize()
        times = []
        for _ in range(args.reps):
            probs, a = pack([w] * n)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch(ctx, probs, a, w.delta, stream)
            e1.record(stream)
            stream.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        res[f"batch_{n}_device_ms"] = ms
        res[f"batch_{n}_problems_per_s"] = n / (ms * 1e-3)
        print(f"batch of {n}: device {ms:.3f} ms per launch (median of {args.reps}), {n / (ms * 1e-3):.0f} problems/s", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
