"""Times dsdtm_clahe_apply_batch (libdsdtm_amd_clahe.so) against clahe_host on one CPU thread.

    python tools/time_clahe.py [--reps 200] [--out FILE]            # the table of profiles/r27_clahe.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_clahe.py --trace     # kernel-only times, a run of its own

Rows, all at 640 x 480, clip limit 3.0, 8 x 8 tiles: one frame device -> device, pinned -> pinned (read in place, read back), pageable ->
pageable (uploaded, read back); 64 and 1024 frames device -> device (distinct sources and destinations). Every call is synchronous (it
ends in the library's wait), so a host clock around it is the call's time; the descriptors are prepared once. Each shape is pre-rolled
before it is timed; medians and the 10th / 90th percentiles are reported. The baseline is clahe_host (dsdtm_amd/host/dsdtm_clahe_host.hpp
at -O2 -ffp-contract=off) on one thread of the same machine over the same frame: this repository's own C++, neither the reference nor
OpenCV.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dsdtm_amd import clahe  # noqa: E402
from tests import clahe_cases as cc  # noqa: E402

W, H = 640, 480


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="a short run for rocprofv3 --kernel-trace: 20 calls at n = 1, 5 each at n = 64 and 1024")
    ap.add_argument("--batches", default="64,1024")
    a = ap.parse_args()
    import torch
    ctx = clahe.ClaheContext(0)          # raises without a gfx950 device: this tool measures on the device
    sizes = [int(v) for v in a.batches.split(",") if v]
    nmax = max(sizes + [1])
    frame = np.ascontiguousarray(cc._textured(W, H, 27))
    want = np.empty_like(frame)
    rng = np.random.default_rng(27)
    src_d = torch.from_numpy(frame).cuda().unsqueeze(0).repeat(nmax, 1, 1).contiguous()
    src_d += torch.from_numpy(rng.integers(0, 3, (nmax, 1, 1), dtype=np.uint8)).cuda()          # (frames differ)
    src_d[0] = torch.from_numpy(frame).cuda()
    dst_d = torch.zeros_like(src_d)
    torch.cuda.synchronize()

    def prepared(frames):
        arr, keep = ctx.descs(frames)
        n = len(frames)

        def call():
            assert ctx.apply_batch_raw(n, arr) == 0, ctx.last_error()
        call.keep = keep
        return call

    dev = {n: prepared([dict(src=src_d[k], dst=dst_d[k]) for k in range(n)]) for n in sorted(set(sizes + [1]))}
    if a.trace:
        for n, calls in [(1, 20)] + [(n, 5) for n in sizes]:
            for _ in range(calls):
                dev[n]()
        print("trace run done")
        return
    host = cc.host_library(tempfile.mkdtemp(prefix="clahe_host_"))
    rows = {}

    def on_host():
        host.clahe_host_c(frame.ctypes.data, W, want.ctypes.data, W, W, H, 3.0, 8, 8, None)
    rows["clahe_host, one thread, n = 1"] = _timed(on_host, max(20, a.reps // 4), 3)
    rows["dsdtm_clahe_apply, device -> device, n = 1"] = _timed(dev[1], a.reps, 10)
    assert np.array_equal(dst_d[0].cpu().numpy(), want)          # (the timed answer is the definition's)
    pin_s, pin_d = torch.from_numpy(frame.copy()).pin_memory(), torch.zeros((H, W), dtype=torch.uint8).pin_memory()
    rows["dsdtm_clahe_apply, pinned -> pinned (read back), n = 1"] = _timed(prepared([dict(src=pin_s, dst=pin_d)]), a.reps, 10)
    assert np.array_equal(pin_d.numpy(), want)
    page_d = np.zeros_like(frame)
    rows["dsdtm_clahe_apply, pageable -> pageable (read back), n = 1"] = _timed(prepared([dict(src=frame, dst=page_d)]), a.reps, 10)
    assert np.array_equal(page_d, want)
    page_to_dev = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rows["dsdtm_clahe_apply, pageable -> device, n = 1"] = _timed(prepared([dict(src=frame, dst=page_to_dev)]), a.reps, 10)
    for n in sizes:
        rows[f"dsdtm_clahe_apply_batch, device -> device, n = {n}"] = _timed(dev[n], max(10, a.reps // max(1, n // 8)), 3)
    base = rows["clahe_host, one thread, n = 1"]["median_us"]
    lines = [f"{'row':<62} {'median us':>11} {'p10':>10} {'p90':>10} {'per frame':>11} {'x host':>8}"]
    for name, r in rows.items():
        n = int(name.rsplit("= ", 1)[1])
        r["per_frame_us"] = r["median_us"] / n
        lines.append(f"{name:<62} {r['median_us']:>11.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f} {r['per_frame_us']:>11.2f} {base / r['per_frame_us']:>8.2f}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(tool="time_clahe", width=W, height=H, rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
