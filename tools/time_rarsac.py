"""Times dsdtm_rarsac_reject_batch (libdsdtm_amd_rarsac.so) against reject_fundamental_host on one CPU thread.

    python tools/time_rarsac.py [--reps 60] [--out FILE]            # the table of profiles/r26_rarsac.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_rarsac.py --trace     # kernel-only times, a run of its own

Rows: the batch entry at n = 1, 64, 1024 with m = 300 correspondences per problem, at 0 % and at 40 % outliers (each problem its own
two-view world: 0.3 px noise, outliers uniform random matches), statuses wanted, default parameters (1000 hypotheses at most, stop at
0.001). Every call is synchronous (it ends in the library's wait), so a host clock around it is the call's time; the descriptors are
prepared once. Each shape is pre-rolled before it is timed; medians and the 10th / 90th percentiles are reported. The baseline is
reject_fundamental_host (dsdtm_amd/host/dsdtm_rarsac_host.hpp at -O2 -ffp-contract=off) on one thread of the same machine over the same
problems: this repository's own C++, neither the reference nor OpenCV.
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

from dsdtm_amd import rarsac  # noqa: E402
from tests import rarsac_cases as rc  # noqa: E402

M, NOISE = 300, 0.3


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


def problems(n, outliers):
    rng = np.random.default_rng(2026 + int(100 * outliers))
    out = []
    for _ in range(n):
        cur, prev, _ = rc.two_views(rng, M, outliers, NOISE)
        out.append(dict(name="timed", cur=cur, prev=prev, width=640, height=480, params={}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="a short run for rocprofv3 --kernel-trace: 20 calls at n = 1, 5 each at n = 64 and 1024")
    ap.add_argument("--batches", default="1,64,1024")
    a = ap.parse_args()
    ctx = rarsac.RarsacContext(0)          # raises without a gfx950 device: this tool measures on the device
    sizes = [int(v) for v in a.batches.split(",") if v]
    if a.trace:
        probs = problems(max(sizes), 0.4)
        for n, calls in ((1, 20), (64, 5), (1024, 5)):
            p = ctx.prepare([dict(cur=c["cur"], prev=c["prev"]) for c in probs[:n]])
            for _ in range(calls):
                assert p.run_raw() == 0, ctx.last_error()
        print("trace run done")
        return
    host = rc.host_library(tempfile.mkdtemp(prefix="rarsac_host_"))
    rows, notes = {}, []
    for outliers in (0.0, 0.4):
        probs = problems(max(sizes), outliers)
        for n in sizes:
            sub = probs[:n]
            tag = f"{int(100 * outliers)} % outliers, n = {n}"

            def on_host():
                for c in sub:
                    rc.run_native(host, c)
            reps = max(5, a.reps // max(1, n // 8))
            r = _timed(on_host, max(3, reps // 4), 1)
            r["per_problem_us"] = r["median_us"] / n
            rows[f"reject_fundamental_host, {tag}"] = r
            p = ctx.prepare([dict(cur=c["cur"], prev=c["prev"]) for c in sub])

            def call():
                assert p.run_raw() == 0, ctx.last_error()
            r = _timed(call, reps, 3)
            r["per_problem_us"] = r["median_us"] / n
            rows[f"dsdtm_rarsac_reject_batch, {tag}"] = r
            ans = p.answers()
            # (the timed answers are the definition's: the first few are held to the host function bit for bit)
            assert all(rc.same(ans[k], rc.run_native(host, sub[k])) for k in range(min(n, 8)))
            notes.append(f"{tag}: mean hypotheses run {statistics.mean(x['iterations_run'] for x in ans):.1f}, mean inliers "
                         f"{statistics.mean(x['n_inliers'] for x in ans):.1f} of {M}")
    lines = [f"{'row':<52} {'median us':>11} {'p10':>10} {'p90':>10} {'per problem':>12} {'x host':>8}"]
    for name, r in rows.items():
        base = rows["reject_fundamental_host, " + name.split(", ", 1)[1]]["per_problem_us"]
        lines.append(f"{name:<52} {r['median_us']:>11.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f} {r['per_problem_us']:>12.2f} {base / r['per_problem_us']:>8.2f}")
    text = "\n".join(lines + notes)
    print(text)
    print(json.dumps(dict(tool="time_rarsac", m=M, rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
