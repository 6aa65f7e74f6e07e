"""Times dsdtm_find_homographies (libdsdtm_amd_homography.so) against its C twin on one CPU thread.

    python tools/time_homography.py [--reps 200] [--out FILE]            # the table of profiles/r16_homography.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_homography.py --trace     # kernel-only times, a run of its own

Rows: the batch entry at n = 1, 64, 1024 with m = 200 correspondences and 40 % outliers per problem (each problem its own points:
0.3 px noise, outliers at least 20 px off), masks wanted. Every call is synchronous (it ends in the library's wait), so a host clock
around it is the call's time; the descriptors are prepared once. Each shape is pre-rolled before it is timed; medians and the 10th /
90th percentiles are reported. The baseline is tests/homography_restatement.c at -O2 -ffp-contract=off on one thread of the same
machine over the same problems: a straightforward C implementation of the same definition, NOT OpenCV.
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

from dsdtm_amd import homography  # noqa: E402
from tests import homography_cases as hc  # noqa: E402

M, OUTLIERS, NOISE = 200, 0.4, 0.3


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


def problems(n):
    rng = np.random.default_rng(2016)
    return [hc._planar(rng, M, OUTLIERS, NOISE)[:2] for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="a short run for rocprofv3 --kernel-trace: 20 calls at n = 1, 5 each at n = 64 and 1024")
    ap.add_argument("--batches", default="1,64,1024")
    a = ap.parse_args()
    ctx = homography.HomographyContext(0)          # raises without a gfx950 device: this tool measures on the device
    sizes = [int(v) for v in a.batches.split(",") if v]
    probs = problems(max(sizes))
    if a.trace:
        for n, calls in ((1, 20), (64, 5), (1024, 5)):
            p = ctx.prepare(probs[:n])
            for _ in range(calls):
                assert p.run_raw() == 0, ctx.last_error()
        print("trace run done")
        return
    lib = hc.c_twin(tempfile.mkdtemp(prefix="homography_twin_"))
    rows, rounds = {}, {}
    for n in sizes:
        sub = probs[:n]

        def twin():
            for A, B in sub:
                hc.run_c(lib, A, B)
        reps = max(5, a.reps // max(1, n // 4))
        r = _timed(twin, max(3, reps // 4), 1)
        r["per_problem_us"] = r["median_us"] / n
        rows[f"C twin -O2, one thread, n = {n}"] = r
        p = ctx.prepare(sub)

        def call():
            assert p.run_raw() == 0, ctx.last_error()
        r = _timed(call, reps, 5)
        r["per_problem_us"] = r["median_us"] / n
        rows[f"dsdtm_find_homographies n = {n}"] = r
        ans = p.answers()
        assert all(x["found"] == 1 for x in ans)
        # (the timed answers are the restatement's: the first few are held to the C twin bit for bit)
        assert all(hc.same(ans[k], hc.run_c(lib, *sub[k])) for k in range(min(n, 8)))
        rounds[n] = (statistics.mean(x["rounds"] for x in ans), statistics.mean(x["refit_iterations"] for x in ans),
                     statistics.mean(x["n_inliers"] for x in ans))
    lines = [f"{'row':<44} {'median us':>11} {'p10':>10} {'p90':>10} {'per problem':>12} {'x C twin':>9}"]
    for name, r in rows.items():
        n = int(name.rsplit("= ", 1)[1])
        base = rows[f"C twin -O2, one thread, n = {n}"]["per_problem_us"]
        lines.append(f"{name:<44} {r['median_us']:>11.1f} {r['p10_us']:>10.1f} {r['p90_us']:>10.1f} {r['per_problem_us']:>12.2f} {base / r['per_problem_us']:>9.2f}")
    for n, (rd, it, inl) in rounds.items():
        lines.append(f"n = {n}: mean rounds {rd:.2f}, mean accepted refit steps {it:.2f}, mean inliers {inl:.1f} of {M}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(dict(tool="time_homography", m=M, outliers=OUTLIERS, rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
